#!/usr/bin/env python3
"""Device time of the Griffin-Lim baseline (csrc/wn_griffin.hip) -> profiles/griffin_timing.json.

    python tools/griffin_timing.py [--out profiles/griffin_timing.json] [--calls 30]

hipEvent medians of `calls` runs after 3 warm-ups (p05 / p95 beside them) of GriffinLim.run_mel with 60 iterations at the default geometry
(2048 / 1100 / 275, 80 mels) for 1 x 5 s and 20 x 5 s of 22.05 kHz; per-iteration time and achieved fp32 TFLOP/s from the counted multiply-adds of the two
products (csrc/wn_griffin.h: gl_frame_macs); beside them the same 60 iterations as a torch.stft / torch.istft loop on the same GPU (rocFFT) and the numpy
float64 host path (datasets.audio, one utterance, extrapolated to the batch); each as a share of the one-shot span (3.147 s) and the folded span (0.332 s)
of 20 x 5 s from the existing profiles.  The shader and memory clocks (rocm-smi --showclocks) are read right after the timed loop of every case."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tacotron-2_amd'))
import hparams as H                     # noqa: E402
from datasets import audio             # noqa: E402
from wavenet_vocoder import _ext      # noqa: E402

ITERS, SR = 60, 22050
ONE_SHOT_S, FOLDED_S = 3.147, 0.332


def clocks():
    try:
        r = subprocess.run(['rocm-smi', '--showclocks'], capture_output=True, text=True, timeout=30)
        return [l.strip() for l in r.stdout.splitlines() if 'sclk' in l or 'mclk' in l][:4]
    except Exception as e:      # noqa: BLE001
        return 'not read (%s)' % type(e).__name__


def events(fn, calls, warm=3):
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


def torch_formulation(S, u, n_fft, win, hop, iters):
    """S, u [B, bins, F] on the device: the same start and iterations on torch.stft / torch.istft"""
    w = torch.hann_window(win, periodic=True, device=S.device)
    n = hop * (S.shape[2] - 1)
    y = torch.istft(torch.polar(S, 2 * np.pi * u), n_fft, hop, win, window=w, center=True, length=n)
    for _ in range(iters):
        X = torch.stft(y, n_fft, hop, win, window=w, center=True, pad_mode='constant', return_complex=True)
        y = torch.istft(torch.polar(S, torch.angle(X)), n_fft, hop, win, window=w, center=True, length=n)
    return y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'griffin_timing.json'))
    ap.add_argument('--calls', type=int, default=30)
    args = ap.parse_args()
    hp = H._build()
    n_fft, win, hop = hp.n_fft, hp.win_size, audio.get_hop_size(hp)
    macs = None
    res = {'what': 'tools/griffin_timing.py: hipEvent medians after 3 warm-ups of GriffinLim.run_mel with %d iterations, geometry (%d, %d, %d), %d mels, 22.05 kHz; '
                   'clocks_after: rocm-smi --showclocks right after the timed loop of the case' % (ITERS, n_fft, win, hop, hp.num_mels),
           'device': torch.cuda.get_device_name(0), 'cases': {}}
    rs = np.random.RandomState(0)
    F = 1 + 5 * SR // hop
    t = np.arange(hop * (F - 1))
    x = 0.3 * np.sin(2 * np.pi * 220.0 * t / SR) * (1 + 0.5 * np.sin(t / 900.0)) + 0.02 * rs.randn(len(t))
    mel1 = audio.melspectrogram(x, hp).astype(np.float32)      # [num_mels, F]
    # multiply-adds of one iteration of one frame, as the kernels run them (the packed formulation over the win_size taps / samples)
    Wp, G, ldi = (win + 7) // 8 * 8, (n_fft // 2 + 31) // 32, (win + 31) // 32 * 32
    macs = Wp * G * 64 + n_fft * ldi
    res['multiply_adds_per_frame_and_iteration'] = macs
    res['square_formulation_multiply_adds'] = 2 * n_fft * n_fft
    t0 = time.perf_counter()
    audio.inv_mel_spectrogram_host([mel1], hp, seed=0)
    host_s = time.perf_counter() - t0
    for B in (1, 20):
        mel = torch.from_numpy(np.repeat(mel1[None], B, 0).copy()).cuda()
        g = _ext.GriffinLim(hp, B, F)
        u = torch.rand((B, F, g.bins), device='cuda')
        out = torch.empty((B, hop * (F - 1)), device='cuda')
        case = {'frames_per_row': F,
                'run_mel_60_iterations': events(lambda: g.run_mel(mel, [F] * B, iters=ITERS, channels_first=True, u=u, out=out), args.calls),
                'start_only': events(lambda: g.run_mel(mel, [F] * B, iters=0, channels_first=True, u=u, out=out), args.calls)}
        it_ms = (case['run_mel_60_iterations']['median_ms'] - case['start_only']['median_ms']) / ITERS
        case['per_iteration_ms'] = it_ms
        case['achieved_fp32_tflops'] = 2.0 * macs * F * B / (it_ms * 1e-3) / 1e12
        S = torch.from_numpy(g.magnitudes(F)).cuda().permute(0, 2, 1).contiguous()
        ut = u.permute(0, 2, 1).contiguous()
        case['torch_stft_istft_60_iterations'] = events(lambda: torch_formulation(S, ut, n_fft, win, hop, ITERS), max(3, args.calls // 3))
        case['run_over_torch'] = case['run_mel_60_iterations']['median_ms'] / case['torch_stft_istft_60_iterations']['median_ms']
        case['numpy_float64_host'] = {'seconds': host_s * B, 'measured_on': '1 utterance, times B'}
        for k in ('run_mel_60_iterations', 'torch_stft_istft_60_iterations'):
            case[k]['share_of_one_shot_span'] = case[k]['median_ms'] * 1e-3 / ONE_SHOT_S
            case[k]['share_of_folded_span'] = case[k]['median_ms'] * 1e-3 / FOLDED_S
        # both loops from the same start: how far apart 60 non-Lipschitz iterations in two arithmetics end, by the convergence each reaches
        g.run_mel(mel, [F] * B, iters=ITERS, channels_first=True, u=u, out=out)      # (the timed start-only runs wrote `out` last)
        yt = torch_formulation(S, ut, n_fft, win, hop, ITERS)
        w = torch.hann_window(win, periodic=True, device='cuda')
        conv = lambda y: float(((torch.stft(y, n_fft, hop, win, window=w, center=True, pad_mode='constant', return_complex=True).abs() - S).norm() / S.norm()).item())
        case['spectral_convergence_after_60'] = {'device': conv(out), 'torch': conv(yt)}
        res['cases']['%d x 5 s' % B] = case
        g.close()
    res['not_measured'] = ['power', 'the kernels under rocprofv3 (where the time of an iteration goes between the two products and the spectrum round trip)',
                           'hop = 256 (the 32-way LDS bank conflict of the forward A operand)', 'more than 20 rows']
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res['cases'], indent=1, sort_keys=True))


if __name__ == '__main__':
    main()
