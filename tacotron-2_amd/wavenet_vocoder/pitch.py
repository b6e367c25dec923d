"""Pitch check: F0 and voicing of generated audio against a recording, per utterance.

    python -m wavenet_vocoder.pitch --generated DIR --reference DIR [--host]

What the reconstruction check cannot see.  An 80-band mel does not resolve harmonics above about 1 kHz and its distances average over a frame, so
pitch drift, octave jumps and voicing that flickers pass it.  Here both signals are tracked by the same estimator (YIN on frames aligned with the mel
frames, csrc/wn_pitch.hip) and the two tracks are compared: the voiced / unvoiced error, the gross pitch error and the F0 error in cents, the three
numbers vocoder evaluations report next to a cepstral distance.  Both signals must be in the same domain: the drivers pre-emphasise the recording as
preprocessing does, so it stands beside the model-domain output; the estimator is scale-invariant, so rescaling needs no care.  What these numbers are for
a trained model is not known here: nobody has one."""
import argparse
import os

import numpy as np

COLUMNS = ('frames', 'voiced_ref', 'voiced_gen', 'both', 'vuv_error', 'gpe', 'f0_rmse_cents', 'f0_bias_cents', 'f0_fine_rmse_cents')
TSV_HEADER = ('name',) + COLUMNS


class PitchCheck(object):
    """One PitchTracker for up to `rows` utterance pairs of up to `max_samples` samples, geometry from the hparams.  tracker: a ready-made one to use
    instead (tests)."""

    def __init__(self, hparams, rows, max_samples, tracker=None):
        from wavenet_vocoder import _ext
        self.rows, self.max_samples = int(rows), int(max_samples)
        self.geometry = _ext.pitch_geometry(hparams)
        self.hop = int(self.geometry['hop'])
        self.tracker = tracker if tracker is not None else _ext.PitchTracker(hparams, self.rows, self.max_samples)

    def score(self, generated, reference, lengths, tracks=False):
        """generated, reference: device float [B, ld] each (ld may differ), both in one domain; row b compares the 1 + lengths[b] // hop frames of its first
        lengths[b] samples.  Both tracks and the comparison run on the device; ONE copy of 9 floats per row brings the result to the host: float32 [B, 9],
        columns COLUMNS (reference first).  tracks: also the device tensors (f0_ref, f0_gen), [B, frames of the longest row] each."""
        lengths = [int(n) for n in lengths]
        frames = [1 + n // self.hop for n in lengths]
        f0_gen = self.tracker.run(generated.float().contiguous(), lengths)[0]
        f0_ref = self.tracker.run(reference.float().contiguous(), lengths)[0]
        table = self.tracker.compare(f0_ref, f0_gen, frames).cpu().numpy()
        return (table, f0_ref, f0_gen) if tracks else table

    def close(self):
        if hasattr(self.tracker, 'close'):
            self.tracker.close()


def tsv_row(name, row):
    vals = [str(int(v)) for v in row[:4]] + ['{:.4f}'.format(float(v)) for v in row[4:6]] + ['{:.2f}'.format(float(v)) for v in row[6:9]]
    return '\t'.join([str(name)] + vals)


def append_tsv(path, names, table):
    """One row per utterance appended to `path` (the header first when the file is new)."""
    new = not os.path.exists(path) or os.path.getsize(path) == 0
    with open(path, 'a', encoding='utf-8') as f:
        if new:
            f.write('\t'.join(TSV_HEADER) + '\n')
        for name, row in zip(names, table):
            f.write(tsv_row(name, row) + '\n')


def read_tsv(path):
    with open(path, encoding='utf-8') as f:
        lines = [l.rstrip('\n').split('\t') for l in f if l.strip()]
    assert tuple(lines[0]) == TSV_HEADER, lines[0]
    return [dict(zip(TSV_HEADER, l)) for l in lines[1:]]


def scalars(row):
    """The three numbers one utterance adds beside the eval loss."""
    pre = 'Wavenet_eval_model/eval_stats/wavenet_eval_'
    return {pre + 'f0_rmse_cents': float(row[6]), pre + 'vuv_error': float(row[4]), pre + 'gpe': float(row[5])}


def log_line(names, table):
    """The batch means, and the worst utterance by voiced / unvoiced error."""
    table = np.asarray(table, dtype=np.float64).reshape(-1, len(COLUMNS))
    w = int(np.argmax(table[:, 4]))
    return ('Pitch check: {} utterance(s), mean V/UV error {:.3f}, gross pitch error {:.3f}, F0 RMSE {:.1f} cents (fine {:.1f}, bias {:+.1f}); worst {} '
            '(V/UV error {:.3f} over {} frames)').format(len(names), table[:, 4].mean(), table[:, 5].mean(), table[:, 6].mean(), table[:, 8].mean(), table[:, 7].mean(),
                                                         names[w], table[w, 4], int(table[w, 0]))


def score_host(generated, reference, hparams):
    """The host evaluation of the same check (the hooks of csrc/wn_pitch.h: the device's arithmetic and order): no GPU.  generated, reference: lists of
    1-D float arrays; pair i compares its first min(len) samples.  -> float32 [N, 9]."""
    from wavenet_vocoder import _ext
    geo = _ext.pitch_geometry(hparams)
    rows = []
    for g, r in zip(generated, reference):
        n = min(len(g), len(r))
        fg = _ext.pitch_host(geo, np.asarray(g, np.float32)[None, :n], [n])['f0']
        fr = _ext.pitch_host(geo, np.asarray(r, np.float32)[None, :n], [n])['f0']
        rows.append(_ext.pitch_compare_host(fr, fg, [fg.shape[1]])[0])
    return np.stack(rows).astype(np.float32) if rows else np.zeros((0, len(COLUMNS)), np.float32)


def score_device(generated, reference, hparams, batch=32):
    """The same pairs on the device, `batch` at a time through one PitchCheck."""
    import torch
    out = np.zeros((len(generated), len(COLUMNS)), np.float32)
    if not generated:
        return out
    lens = [min(len(g), len(r)) for g, r in zip(generated, reference)]
    chk = PitchCheck(hparams, min(batch, len(lens)), max(lens))
    try:
        for lo in range(0, len(lens), chk.rows):
            idx = list(range(lo, min(lo + chk.rows, len(lens))))
            ld = max(max(lens[i] for i in idx), 1)
            g, r = np.zeros((len(idx), ld), np.float32), np.zeros((len(idx), ld), np.float32)
            for k, i in enumerate(idx):
                g[k, :lens[i]] = np.asarray(generated[i], np.float32)[:lens[i]]
                r[k, :lens[i]] = np.asarray(reference[i], np.float32)[:lens[i]]
            out[idx] = chk.score(torch.from_numpy(g).cuda(), torch.from_numpy(r).cuda(), [lens[i] for i in idx])
    finally:
        chk.close()
    return out


def read_pairs(generated_dir, reference_dir):
    """(name, generated path, reference path) of every wav of generated_dir with a wav of the same name in reference_dir (a ``wavenet-audio-`` prefix of
    the generated name does not count), and how many were skipped."""
    pairs, skipped = [], 0
    for n in sorted(os.listdir(generated_dir)):
        if not n.endswith('.wav'):
            continue
        cands = [n] + ([n[len('wavenet-audio-'):]] if n.startswith('wavenet-audio-') else [])
        ref = next((c for c in cands if os.path.exists(os.path.join(reference_dir, c))), None)
        if ref is None:
            skipped += 1
            continue
        pairs.append((ref[:-4], os.path.join(generated_dir, n), os.path.join(reference_dir, ref)))
    return pairs, skipped


def main(argv=None):
    from datasets import audio
    import hparams as H
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--generated', required=True, help='directory of generated wavs')
    ap.add_argument('--reference', required=True, help='directory of recordings of equal names')
    ap.add_argument('--tsv', default=None, help='append the table here (the format of wavs/pitch.tsv)')
    ap.add_argument('--host', action='store_true', help='evaluate on the host (the hooks: the same arithmetic): no GPU; the default is the device')
    ap.add_argument('--hparams', default='', help='comma separated name=value overrides')
    args = ap.parse_args(argv)
    hp = H._build().parse(args.hparams)          # a copy: the process-wide defaults stay as they are
    pairs, skipped = read_pairs(args.generated, args.reference)
    if skipped:
        print('skipped {} generated wav file(s) without a recording of the same name'.format(skipped))
    if not pairs:
        raise RuntimeError('no wav pairs of equal names found')
    gen = [audio.load_wav(g, sr=hp.sample_rate) for _, g, _ in pairs]          # files of both folders are taken as they are: one domain is the caller's business
    ref = [audio.load_wav(r, sr=hp.sample_rate) for _, _, r in pairs]
    table = (score_host if args.host else score_device)(gen, ref, hp)
    names = [n for n, _, _ in pairs]
    print('\t'.join(TSV_HEADER))
    for n, row in zip(names, table):
        print(tsv_row(n, row))
    print(log_line(names, table))
    if args.tsv:
        append_tsv(args.tsv, names, table)
    return names, table


if __name__ == '__main__':
    main()
