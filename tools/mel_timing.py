#!/usr/bin/env python3
"""Device time of the mel analysis (wn_mel_run, csrc/wn_mel.hip) -> profiles/mel_timing.json, and the parity ratios of tests/test_hip_mel.py
-> profiles/mel_parity.json.

    python tools/mel_timing.py [--repeats 20] [--out profiles/mel_timing.json] [--parity-out profiles/mel_parity.json]

Cases: 1 x 5 s, 20 x 9 s (900 frames = max_mel_frames) and 64 x 9 s of noise at the default geometry.  Per case and frame tile (the
WN_MEL_TF switch of wn_mel_create: 32 / 64 / 128 frames per workgroup): median, min and max over `repeats` event-bracketed calls after 3
warm-up calls, and the achieved fp32 FLOP/s (useful FLOPs: 2 x win x 2 x bins + 2 x bins x mels per frame) against the 157 TFLOP/s
nameplate of the fp32 matrix instruction.  Yardsticks: (a) datasets.audio.melspectrogram (numpy float64) on this host, timed per
utterance and scaled to the batch; (b) a torch.stft (rocFFT) formulation of the same analysis on the same GPU, if it runs."""
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

NAMEPLATE_FP32_MATRIX = 157.3e12


def _events(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    q = statistics.quantiles(ms, n=4)
    return {'median_ms': statistics.median(ms), 'min_ms': min(ms), 'max_ms': max(ms), 'q1_ms': q[0], 'q3_ms': q[2], 'repeats': repeats}


def _clocks():
    try:
        r = subprocess.run(['rocm-smi', '--showclocks'], capture_output=True, text=True, timeout=30)
        return [l.strip() for l in r.stdout.splitlines() if 'sclk' in l or 'mclk' in l][:4]
    except Exception as e:      # noqa: BLE001
        return 'not read (%s)' % type(e).__name__


def _stft_yardstick(hp, wav, lens, basis):
    """the same analysis through torch.stft: zero-padded centred frames, periodic Hann of win_size, |.|^2, mel filters, level, normalisation"""
    win = torch.hann_window(hp.win_size, periodic=True, device=wav.device)
    mb = torch.from_numpy(basis).to(wav.device)
    min_lin = 10.0 ** (hp.min_level_db / 20)

    def run():
        D = torch.stft(wav, hp.n_fft, hop_length=hp.hop_size, win_length=hp.win_size, window=win, center=True, pad_mode='constant', return_complex=True)
        P = D.real * D.real + D.imag * D.imag
        S = 20 * torch.log10(torch.clamp_min(torch.matmul(mb, P), min_lin)) - hp.ref_level_db
        return torch.clamp((2 * hp.max_abs_value) * ((S - hp.min_level_db) / (-hp.min_level_db)) - hp.max_abs_value, -hp.max_abs_value, hp.max_abs_value)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mel_timing.json'))
    ap.add_argument('--parity-out', default=os.path.join(ROOT, 'profiles', 'mel_parity.json'))
    ap.add_argument('--skip-parity', action='store_true')
    args = ap.parse_args()
    from datasets import audio
    from mel_util import mel_hparams
    from wavenet_vocoder import _ext
    hp = mel_hparams()
    hop, nb = hp.hop_size, 1 + hp.n_fft // 2
    flops_per_frame = 2.0 * hp.win_size * 2 * nb + 2.0 * nb * hp.num_mels
    basis = audio._build_mel_basis(hp)
    props = torch.cuda.get_device_properties(0)
    report = {'device': props.name, 'compute_units': props.multi_processor_count, 'nameplate_fp32_matrix_flops': NAMEPLATE_FP32_MATRIX,
              'geometry': {'n_fft': hp.n_fft, 'hop_size': hop, 'win_size': hp.win_size, 'num_mels': hp.num_mels}, 'flops_per_frame': flops_per_frame,
              'method': 'HIP events around one wn_mel_run on the current stream, 3 warm-up calls, median / min / max over the repeats', 'cases': []}
    rng = np.random.RandomState(0)
    for name, B, n in (('1x5s', 1, 5 * hp.sample_rate), ('20x9s', 20, 899 * hop + 100), ('64x9s', 64, 899 * hop + 100)):
        host = (0.1 * rng.randn(B, n)).astype(np.float32)
        wav = torch.from_numpy(host).cuda()
        lens = [n] * B
        frames = B * (1 + n // hop)
        case = {'case': name, 'batch': B, 'samples': n, 'frames': frames, 'tiles': {}}
        outs = {}
        for tf in (32, 64, 128, 'auto'):      # 'auto': the library's own per-call choice (what a user gets)
            os.environ.pop('WN_MEL_TF', None)
            if tf != 'auto':
                os.environ['WN_MEL_TF'] = str(tf)
            an = _ext.MelAnalyzer(hp, B, n)
            assert an.frame_tile == (128 if tf == 'auto' else tf)
            out = torch.empty(B, 1 + n // hop, hp.num_mels, device='cuda')
            t = _events(lambda: an.run(wav, lens, out=out), 3, args.repeats)
            t['tflops'] = frames * flops_per_frame / (t['median_ms'] * 1e-3) / 1e12
            t['fraction_of_nameplate'] = t['tflops'] * 1e12 / NAMEPLATE_FP32_MATRIX
            case['tiles'][str(tf)] = t
            outs[tf] = out.cpu().numpy()
            an.close()
            print('%-6s TF=%4s  %.3f ms (min %.3f max %.3f)  %.1f TFLOP/s' % (name, tf, t['median_ms'], t['min_ms'], t['max_ms'], t['tflops']), flush=True)
        case['clocks_right_after_the_timed_calls'] = _clocks()      # read-only; the device idles down within milliseconds, so this bounds nothing from above
        os.environ.pop('WN_MEL_TF', None)
        case['max_abs_difference_between_tiles'] = float(max(np.max(np.abs(outs[t] - outs[64])) for t in (32, 128, 'auto')))
        # (a) numpy float64 on this host, per utterance
        k = min(B, 2)
        t0 = time.perf_counter()
        for b in range(k):
            ref = audio.melspectrogram(host[b].astype(np.float64), hp)
        per = (time.perf_counter() - t0) / k
        case['numpy_float64_host'] = {'ms_per_utterance': per * 1e3, 'ms_for_batch_scaled': per * 1e3 * B, 'utterances_timed': k, 'host_threads_available': len(os.sched_getaffinity(0)), 'omp_num_threads': os.environ.get('OMP_NUM_THREADS')}
        case['device_vs_numpy_max_abs'] = float(np.max(np.abs(outs[64][k - 1].T - ref)))
        # (b) torch.stft on the same GPU
        try:
            run = _stft_yardstick(hp, wav, lens, basis)
            y = run()
            t = _events(run, 3, args.repeats)
            t['max_abs_vs_device_kernel'] = float((y.transpose(1, 2) - torch.from_numpy(outs[64]).cuda()).abs().max())
            case['torch_stft_same_gpu'] = t
            print('%-6s torch.stft  %.3f ms' % (name, t['median_ms']), flush=True)
        except Exception as e:      # noqa: BLE001
            case['torch_stft_same_gpu'] = 'not usable here: %s: %s' % (type(e).__name__, str(e).splitlines()[0][:200])
            print('%-6s torch.stft not usable: %s' % (name, e), flush=True)
        report['cases'].append(case)
        with open(args.out, 'w') as f:
            json.dump(report, f, indent=1)
    if not args.skip_parity:
        from mel_util import CONFIGS, TILES, check_parity
        rows = []
        for tile in (None,) + TILES:
            rows += check_parity(hp, 'default', tile=tile)
        for label, over in CONFIGS:
            for tile in TILES:
                rows += check_parity(mel_hparams(**over), label, max_frames=300, tile=tile)
        with open(args.parity_out, 'w') as f:
            json.dump({'bound': 'device error <= 8 x max(float32 yardstick, 2^-19)', 'max_ratio': max(r['ratio_to_floored_yardstick'] for r in rows),
                       'rows': rows}, f, indent=1)
        print('parity: max ratio %.2f over %d rows' % (max(r['ratio_to_floored_yardstick'] for r in rows), len(rows)))


if __name__ == '__main__':
    main()
