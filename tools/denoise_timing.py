#!/usr/bin/env python3
"""Device time of the spectral denoiser (csrc/wn_denoise.hip) -> profiles/denoise_timing.json.

    python tools/denoise_timing.py [--out profiles/denoise_timing.json]

hipEvent medians of 30 calls after 3 warm-ups (p05 / p95 beside them) of SpectralDenoiser.apply and .fit at 1 x 5 s and 20 x 5 s of 22.05 kHz in the default
geometry (1024, 256); beside them the same operation as a torch.stft / torch.istft formulation on the same GPU (rocFFT) and as scipy stft / istft in float64
on the host with the .cpu() copy it needs; each as a share of the one-shot span (3.147 s) and the folded span (0.332 s) of 20 x 5 s from the existing
profiles.  The shader and memory clocks (rocm-smi --showclocks) are read right after the timed loop of every case and stored beside it."""
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
from wavenet_vocoder import _ext      # noqa: E402

N_FFT, HOP, SR = 1024, 256, 22050
ONE_SHOT_S, FOLDED_S = 3.147, 0.332


def clocks():
    try:
        r = subprocess.run(['rocm-smi', '--showclocks'], capture_output=True, text=True, timeout=30)
        return [l.strip() for l in r.stdout.splitlines() if 'sclk' in l or 'mclk' in l][:4]
    except Exception as e:      # noqa: BLE001
        return 'not read (%s)' % type(e).__name__


def events(fn, calls=30, warm=3):
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


def torch_formulation(x, prof, strength):
    w = torch.hann_window(N_FFT, periodic=True, device=x.device)
    X = torch.stft(x, N_FFT, HOP, window=w, center=True, pad_mode='constant', return_complex=True)
    m = X.abs()
    t = strength * prof[None, :, None]
    Y = X * torch.where(m > t, (m - t) / m.clamp_min(1e-30), torch.zeros_like(m))
    return torch.istft(Y, N_FFT, HOP, window=w, center=True, length=x.shape[1])


def scipy_host(x_dev, prof, strength):
    from scipy import signal
    x = x_dev.cpu().numpy().astype(np.float64)
    _, _, Z = signal.stft(x, window='hann', nperseg=N_FFT, noverlap=N_FFT - HOP, boundary='zeros')
    m = np.abs(Z)
    t = strength * prof[None, :, None] / np.hanning(N_FFT + 1)[:-1].sum()
    Z = Z * np.where(m > t, (m - t) / np.maximum(m, 1e-300), 0.0)
    return signal.istft(Z, window='hann', nperseg=N_FFT, noverlap=N_FFT - HOP, boundary=True)[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'denoise_timing.json'))
    args = ap.parse_args()
    res = {'what': 'tools/denoise_timing.py: hipEvent medians of 30 calls after 3 warm-ups, geometry (1024, 256), 22.05 kHz; clocks_after: rocm-smi --showclocks right after the timed loop of the case',
           'device': torch.cuda.get_device_name(0), 'cases': {}}
    rs = np.random.RandomState(0)
    for B in (1, 20):
        n = 5 * SR
        x = torch.from_numpy((0.1 * rs.randn(B, n)).astype(np.float32)).cuda()
        d = _ext.SpectralDenoiser(N_FFT, HOP, B, n)
        d.fit(x, [n] * B)
        prof = torch.from_numpy(d.profile).cuda()
        out = torch.empty_like(x)
        case = {'run': events(lambda: d.apply(x, [n] * B, 1.0, out=out)), 'fit': events(lambda: d.fit(x, [n] * B)),
                'torch_stft_istft': events(lambda: torch_formulation(x, prof, 1.0))}
        t0 = time.perf_counter()
        for _ in range(3):
            scipy_host(x, d.profile.astype(np.float64), 1.0)
        case['scipy_float64_host_with_cpu_copy'] = {'mean_ms': (time.perf_counter() - t0) / 3 * 1e3, 'calls': 3}
        ref = torch_formulation(x, prof, 1.0)
        case['max_abs_difference_from_torch_formulation'] = float((out - ref)[:, N_FFT:-N_FFT].abs().max())
        for k in ('run', 'fit', 'torch_stft_istft'):
            case[k]['share_of_one_shot_span'] = case[k]['median_ms'] * 1e-3 / ONE_SHOT_S
            case[k]['share_of_folded_span'] = case[k]['median_ms'] * 1e-3 / FOLDED_S
        case['run_over_torch'] = case['run']['median_ms'] / case['torch_stft_istft']['median_ms']
        res['cases']['%d x 5 s' % B] = case
        d.close()
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res['cases'], indent=1, sort_keys=True))


if __name__ == '__main__':
    main()
