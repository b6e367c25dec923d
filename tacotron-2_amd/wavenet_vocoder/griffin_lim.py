"""``python -m wavenet_vocoder.griffin_lim (--map training_data/map.txt | --mels DIR) --output_dir OUT [--iters N] [--seed S] [--host]``: every mel of a
preprocessed folder (the mel column of map.txt, or every ``*.npy`` of a directory; [frames, num_mels] as preprocessing writes them) inverted WITHOUT a
model -- the pseudo-inverse of the mel filters, ** power, Griffin-Lim (reference datasets/audio.py:97-112; the job of its griffin_lim_synthesis_tool
notebook: "choose how good your preprocessing is") -- one ``griffin-lim-<name>.wav`` per mel under OUT.  Ragged batches run on the device
(csrc/wn_griffin.hip); ``--host`` or ``GL_on_GPU=False`` takes the numpy float64 path and needs no GPU."""
import argparse
import os
import time

import numpy as np

from datasets import audio
from hparams import hparams as default_hparams


def mel_files(args):
    """[(name, path)] in map.txt row order / sorted file names"""
    if args.map:
        base = os.path.dirname(os.path.abspath(args.map))
        with open(args.map, encoding='utf-8') as f:
            rows = [line.strip().split('|') for line in f if line.strip()]
        paths = [r[1] if os.path.isabs(r[1]) or os.path.exists(r[1]) else os.path.join(base, 'mels', os.path.basename(r[1])) for r in rows]      # audio|mel|...
    else:
        paths = sorted(os.path.join(args.mels, n) for n in os.listdir(args.mels) if n.endswith('.npy'))
    out = []
    for p in paths:
        name = os.path.basename(p)[:-len('.npy')]
        out.append((name[len('mel-'):] if name.startswith('mel-') else name, p))
    return out


def run(args, hparams):
    files = mel_files(args)
    if not files:
        raise RuntimeError('no mel found')
    os.makedirs(args.output_dir, exist_ok=True)
    if args.iters is not None:
        hparams.griffin_lim_iters = int(args.iters)
    host = bool(args.host) or not bool(getattr(hparams, 'GL_on_GPU', True))
    mels = []
    for name, p in files:
        m = np.load(p)
        if m.ndim != 2 or m.shape[1] != hparams.num_mels:
            raise ValueError('{}: expected [frames, {}], got {}'.format(p, hparams.num_mels, m.shape))
        if m.shape[0] < 2:
            raise ValueError('{}: a mel of {} frame(s) has no Griffin-Lim signal'.format(p, m.shape[0]))
        mels.append(np.ascontiguousarray(m.T, dtype=np.float32))
    t0 = time.time()
    if host:
        wavs = audio.inv_mel_spectrogram_host(mels, hparams, seed=args.seed)
    else:
        wavs = audio.inv_mel_spectrogram_device(mels, None, hparams, seed=args.seed)
    dt = time.time() - t0
    paths = []
    for (name, _), w in zip(files, wavs):
        paths.append(os.path.join(args.output_dir, 'griffin-lim-{}.wav'.format(name)))
        audio.save_wavenet_wav(w, paths[-1], sr=hparams.sample_rate)
    seconds = sum(len(w) for w in wavs) / float(hparams.sample_rate)
    print('Griffin-Lim ({}): {} mel(s), {} iterations, {:.1f} s of audio in {:.2f} s -> {}'.format('numpy' if host else 'device', len(wavs), int(hparams.griffin_lim_iters),
                                                                                                 seconds, dt, args.output_dir))
    return paths


def main(argv=None):
    ap = argparse.ArgumentParser(description='mel -> wav without a model (Griffin-Lim): audit a preprocessed or GTA mel folder by ear')
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument('--map', help='training_data/map.txt (audio|mel|... rows; the mels lie in mels/ beside it)')
    src.add_argument('--mels', help='a directory of *.npy mels [frames, num_mels]')
    ap.add_argument('--output_dir', required=True)
    ap.add_argument('--iters', type=int, default=None, help='Griffin-Lim iterations after the start (default: hparams.griffin_lim_iters)')
    ap.add_argument('--seed', type=int, default=0, help='seed of the random start')
    ap.add_argument('--host', action='store_true', help='the numpy float64 path: no GPU')
    ap.add_argument('--hparams', default='', help='comma separated name=value overrides')
    args = ap.parse_args(argv)
    hp = default_hparams.parse(args.hparams) if args.hparams else default_hparams
    return run(args, hp)


if __name__ == '__main__':
    main()
