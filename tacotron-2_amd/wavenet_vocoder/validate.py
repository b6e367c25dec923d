"""Score a data set with a trained WaveNet: the held-out negative log-likelihood per sample, per utterance and in total.

    python -m wavenet_vocoder.validate --checkpoint DIR --input map.txt [--ema] [--json FILE] [--split all|test] [--hparams ...]

The checkpoint is restored into a context of its own; every utterance of the metadata file (``--split test``: of the test split the
training run holds out) goes once through a batched, dropout-free, teacher-forced forward (WaveNet.validate) with the crops of
``Feeder.validation_batches`` -- the numbers of a training run's ``mi355_validation_interval`` lines, reproducible from the checkpoint.
Prints the aggregate loss (the training definition) and the ten worst utterances; ``--json`` writes the per-utterance table."""
import argparse
import json
import os

import torch

from datasets import audio
from hparams import hparams as default_hparams
from wavenet_vocoder.feeder import Feeder
from wavenet_vocoder.models import create_model
from wavenet_vocoder.train import get_checkpoint_state


def find_checkpoint(path):
    """A checkpoint file, a wave_pretrained directory (its index names the newest file) or a log directory that holds one."""
    if os.path.isfile(path):
        return path
    for d in (path, os.path.join(path, 'wave_pretrained')):
        ckpt = get_checkpoint_state(d) if os.path.isdir(d) else None
        if ckpt and os.path.exists(ckpt):
            return ckpt
    raise FileNotFoundError('no checkpoint at {}'.format(path))


def score(checkpoint, input_path, hparams, base_dir='', ema=False, split='all'):
    """-> (summary dict of WaveNet.validate, [audio path of every utterance, in the order of summary['utterances']])."""
    feeder = Feeder(None, os.path.join(base_dir, input_path), base_dir, hparams)
    groups = feeder.validation_utterances(split)
    names = [meta[0] for group in groups for _, meta in group]
    if not names:
        raise ValueError('no utterance to score in {} (split={})'.format(input_path, split))
    hop = audio.get_hop_size(hparams)
    limit = int(hparams.max_time_sec * hparams.sample_rate) if hparams.max_time_sec is not None else hparams.max_time_steps
    lengths = [feeder._length_of(n) for n in names]
    max_t = max(n if (limit is None or n <= limit) else limit - limit % hop for n in lengths)      # (_limit_time's crop)
    model = create_model('WaveNet', hparams)
    model.build(max(len(g) for g in groups), max(max_t, hop * 2))
    model.load_state_dict(torch.load(find_checkpoint(checkpoint), map_location='cpu'))
    if ema:
        model.use_ema_weights()
    return model.validate(feeder.validation_batches(split)), names


def table(summary, names):
    """One row per utterance: audio path, samples scored, sum and per-sample mean of the negative log-likelihood (nats)."""
    return [{'audio': n, 'samples': c, 'nonzero': z, 'nll_sum': s, 'nll_per_sample': (s / c if c > 0 else None)}
            for n, (s, c, z) in zip(names, summary['utterances'])]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--checkpoint', required=True, help='checkpoint file, wave_pretrained directory or log directory')
    ap.add_argument('--input', required=True, help='metadata file (map.txt of wavenet_preprocess)')
    ap.add_argument('--base_dir', default='')
    ap.add_argument('--ema', action='store_true', help='score the EMA weights instead of the raw ones')
    ap.add_argument('--split', default='all', choices=('all', 'test'), help="'test': only the split the training run holds out")
    ap.add_argument('--json', default=None, help='write the per-utterance table here')
    ap.add_argument('--hparams', default='', help='comma separated name=value overrides')
    args = ap.parse_args(argv)
    hp = default_hparams.parse(args.hparams)
    summary, names = score(args.checkpoint, args.input, hp, base_dir=args.base_dir, ema=args.ema, split=args.split)
    rows = table(summary, names)
    print('Validation loss: {:.5f} ({} utterances, {} samples{})'.format(summary['loss'], len(rows), summary['count'], ', EMA weights' if args.ema else ''))
    worst = sorted((r for r in rows if r['nll_per_sample'] is not None), key=lambda r: -r['nll_per_sample'])[:10]
    print('Worst utterances (nats per sample):')
    for r in worst:
        print('  {:10.5f}  {:8d} samples  {}'.format(r['nll_per_sample'], r['samples'], r['audio']))
    if args.json:
        with open(args.json, 'w') as f:
            json.dump({'loss': summary['loss'], 'sum': summary['sum'], 'count': summary['count'], 'nonzero': summary['nonzero'], 'ema': bool(args.ema),
                       'utterances': rows}, f, indent=1)
    return summary


if __name__ == '__main__':
    main()
