"""WaveNet preprocessing CLI: a folder of wav files -> the dataset ``train.py --model WaveNet`` reads.

    python wavenet_preprocess.py --input_dir LJSpeech-1.1/wavs --output training_data

Flags, defaults and outputs follow the reference's program of the same name (--base_dir --hparams --input_dir --output --n_jobs): under
<base_dir>/<output>/ it writes audio/audio-<name>.npy, mels/mel-<name>.npy and map.txt with one row
``audio|mel|mel|<no_g>|time_steps|mel_frames`` per kept utterance, in sorted file order.  The mel analysis runs on the GPU (hparams
mi355_device_mel, which this program turns on unless --hparams sets it; ``mi355_device_mel=False`` analyses in numpy and needs no GPU)."""
import argparse
import os

from hparams import hparams

MAP_COLUMNS = ('audio', 'mel', 'gta_mel', 'speaker', 'time_steps', 'mel_frames')


def save_map(rows, dataset_dir):
    """rows of datasets.wavenet_preprocessor.build_from_path -> <dataset_dir>/map.txt, columns MAP_COLUMNS joined by '|'"""
    lines = ['|'.join(str(col) for col in row) for row in rows]
    assert all(len(row) == len(MAP_COLUMNS) for row in rows)
    with open(os.path.join(dataset_dir, 'map.txt'), 'w', encoding='utf-8') as f:
        f.write(''.join(line + '\n' for line in lines))
    return len(lines)


def report(rows, sample_rate):
    if not rows:
        print('no utterance was kept')
        return
    samples = [int(r[MAP_COLUMNS.index('time_steps')]) for r in rows]
    frames = [int(r[MAP_COLUMNS.index('mel_frames')]) for r in rows]
    print('%d utterances kept: %d samples = %.2f h of audio; longest utterance %d samples / %d frames'
          % (len(rows), sum(samples), sum(samples) / float(sample_rate) / 3600.0, max(samples), max(frames)))


def run(hp, input_dir, dataset_dir, n_jobs):
    from tqdm import tqdm
    from datasets.wavenet_preprocessor import build_from_path
    sub = {name: os.path.join(dataset_dir, name) for name in ('mels', 'audio')}
    for d in sub.values():
        os.makedirs(d, exist_ok=True)
    rows = build_from_path(hp, input_dir, sub['mels'], sub['audio'], n_jobs, tqdm=tqdm)
    save_map(rows, dataset_dir)
    report(rows, hp.sample_rate)
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--base_dir', default='', help='prefix of --output')
    ap.add_argument('--hparams', default='', help='comma-separated name=value overrides of hparams.py')
    ap.add_argument('--input_dir', default='LJSpeech-1.1/wavs', help='folder of *.wav at hparams.sample_rate')
    ap.add_argument('--output', default='tacotron_output/gta/', help='dataset folder (audio/, mels/, map.txt), under --base_dir')
    ap.add_argument('--n_jobs', type=int, default=min(os.cpu_count() or 1, 16), help='worker processes of the host steps')
    args = ap.parse_args(argv)
    hp = hparams.parse(args.hparams)
    if 'mi355_device_mel' not in args.hparams:      # on for this program unless the caller decides
        hp.mi355_device_mel = True
    run(hp, args.input_dir, os.path.join(args.base_dir, args.output), args.n_jobs)


if __name__ == '__main__':
    main()
