"""Reconstruction check: how far the mel-spectrogram of generated audio is from the mel it was generated from, per frame and per utterance.

    python -m wavenet_vocoder.reconstruction --map wavs/map.txt
    python -m wavenet_vocoder.reconstruction --wavs DIR --mels DIR

The number behind the "Local Condition vs Reconst. Mel-Spectrogram" plot.  The generated signal is analysed exactly as preprocessing analyses a
recording (the pre-emphasis fused into the analysis, csrc/wn_mel.hip) and compared with its conditioning on the device (csrc/wn_melcmp.hip).
Preprocessing rescales the network's target and the pre-emphasised signal the mel is made of independently, so even a perfect vocoder shows one
constant level offset per utterance: it is reported as bias_db, and the distances one reads -- l1c_db, lsdc_db -- have the utterance's own bias
removed; mcd_db leaves out the level coefficient.  What these numbers are for a trained model is not known here: nobody has one."""
import argparse
import os

import numpy as np

COLUMNS = ('bias_db', 'l1_db', 'lsd_db', 'mcd_db', 'l1c_db', 'lsdc_db', 'worst_db', 'worst_frame', 'alarm_frames')
TSV_HEADER = ('name', 'frames') + COLUMNS
N_CEP = 13


def n_cep_for(num_mels):
    return min(N_CEP, int(num_mels) - 1)


class ReconstructionCheck(object):
    """One MelAnalyzer and one MelCompare for up to `rows` utterances of up to `max_samples` samples: geometry and unit_db from the hparams,
    channels-first analysis, the pre-emphasis of preprocessing (hparams.preemphasis if hparams.preemphasize else 0) fused into it.  analyzer / compare:
    ready-made stages to use instead (tests)."""

    def __init__(self, hparams, rows, max_samples, preemphasis=None, alarm_db=None, analyzer=None, compare=None):
        from datasets.audio import get_hop_size
        from wavenet_vocoder import _ext
        if int(hparams.cin_channels) != int(hparams.num_mels):
            raise ValueError('reconstruction check: the conditioning has cin_channels = {} channels, the analysis num_mels = {}: nothing to compare'.format(
                hparams.cin_channels, hparams.num_mels))
        self.hop, self.num_mels = int(get_hop_size(hparams)), int(hparams.num_mels)
        self.rows, self.max_samples = int(rows), int(max_samples)
        if preemphasis is None:
            preemphasis = float(hparams.preemphasis) if hparams.preemphasize else 0.0
        if alarm_db is None:
            alarm_db = float(getattr(hparams, 'mi355_reconstruction_alarm_db', 6.0))
        self.preemphasis, self.alarm_db, self.unit_db = float(preemphasis), float(alarm_db), _ext.melcmp_unit_db(hparams)
        self.analyzer = analyzer if analyzer is not None else _ext.MelAnalyzer(hparams, self.rows, self.max_samples, preemphasis=self.preemphasis)
        self.compare = compare if compare is not None else _ext.MelCompare(self.num_mels, self.rows, 1 + self.max_samples // self.hop, n_cep=n_cep_for(self.num_mels),
                                                                           unit_db=self.unit_db, alarm_db=self.alarm_db)

    def score(self, wav, lengths, c, frames=None, per_frame=False, c_channels_first=True):
        """wav: device float [B, ld], decoded model-domain samples (not de-emphasised), row b holds lengths[b]; c: device float [B, cin, Tc]
        (c_channels_first=False: [B, Tc, cin]), in the scale the analysis writes (hparams' mel normalisation).  frames: per row, how many to compare
        (default lengths[b] // hop: the analysis of Tc * hop samples has Tc + 1 frames, frame f of both is centred on sample f * hop, the extra one is
        not compared).  Analysis and comparison run on the device; ONE copy brings the result to the host: float32 [B, 9], columns COLUMNS.  per_frame:
        also the device tensor [B, 6, frames] (bias, l1, lsd, mcd, l1c, lsdc)."""
        import torch
        lengths = [int(n) for n in lengths]
        if c.dim() != 3 or int(c.shape[1 if c_channels_first else 2]) != self.num_mels:
            raise ValueError('reconstruction check: c must be {} with {} channels (got {})'.format('[B, cin, Tc]' if c_channels_first else '[B, Tc, cin]', self.num_mels, tuple(c.shape)))
        Tc = int(c.shape[2 if c_channels_first else 1])
        if frames is None:
            frames = [n // self.hop for n in lengths]
        frames = [int(f) for f in frames]
        for b, (f, n) in enumerate(zip(frames, lengths)):
            if f > Tc or f > 1 + n // self.hop:
                raise ValueError('reconstruction check: row {} compares {} frames, but has {} of conditioning and {} of signal'.format(b, f, Tc, 1 + n // self.hop))
        a = self.analyzer.run(wav, lengths, channels_first=True)
        res = self.compare.run(a, c.float().contiguous(), frames, a_channels_first=True, b_channels_first=c_channels_first, per_frame=per_frame)
        table = torch.cat((res['summary'], res['marks'].to(torch.float32)), dim=1).cpu().numpy()      # (frame indices and counts are exact in float32 below 2^24)
        return (table, res['per_frame']) if per_frame else table

    def close(self):
        for st in (self.analyzer, self.compare):
            if hasattr(st, 'close'):
                st.close()


def tsv_row(name, frames, row):
    vals = ['{:.4f}'.format(float(v)) for v in row[:7]] + [str(int(row[7])), str(int(row[8]))]
    return '\t'.join([str(name), str(int(frames))] + vals)


def append_tsv(path, names, frames, table):
    """One row per utterance appended to `path` (the header first when the file is new)."""
    new = not os.path.exists(path) or os.path.getsize(path) == 0
    with open(path, 'a', encoding='utf-8') as f:
        if new:
            f.write('\t'.join(TSV_HEADER) + '\n')
        for name, fr, row in zip(names, frames, table):
            f.write(tsv_row(name, fr, row) + '\n')


def read_tsv(path):
    with open(path, encoding='utf-8') as f:
        lines = [l.rstrip('\n').split('\t') for l in f if l.strip()]
    assert tuple(lines[0]) == TSV_HEADER, lines[0]
    return [dict(zip(TSV_HEADER, l)) for l in lines[1:]]


def log_line(names, table):
    """The batch means of the level-compensated distances, and the worst utterance by l1c_db."""
    table = np.asarray(table, dtype=np.float64).reshape(-1, len(COLUMNS))
    w = int(np.argmax(table[:, 4]))
    return ('Reconstruction check: {} utterance(s), mean bias {:+.2f} dB, l1c {:.2f} dB, lsdc {:.2f} dB, mcd {:.2f} dB; worst {} (l1c {:.2f} dB, frame {} at {:.2f} dB, '
            '{} alarmed frames)').format(len(names), table[:, 0].mean(), table[:, 4].mean(), table[:, 5].mean(), table[:, 3].mean(), names[w], table[w, 4],
                                         int(table[w, 7]), table[w, 6], int(table[w, 8]))


def score_host(wavs, mels, hparams, alarm_db=None):
    """The host evaluation of the same check (numpy analysis in float64, wn_test_melcmp_host for the distances): no GPU.  wavs: 1-D float arrays; mels:
    [Tc, num_mels] each.  -> (frames per pair, float32 [N, 9])."""
    from datasets import audio
    from wavenet_vocoder import _ext
    if alarm_db is None:
        alarm_db = float(getattr(hparams, 'mi355_reconstruction_alarm_db', 6.0))
    hop, M = audio.get_hop_size(hparams), int(hparams.num_mels)
    frames, rows = [], []
    for wav, mel in zip(wavs, mels):
        x = audio.preemphasis(np.asarray(wav, dtype=np.float64), hparams.preemphasis, hparams.preemphasize)
        a = audio.melspectrogram(x, hparams).astype(np.float32)                    # [M, 1 + n // hop]
        F = min(len(mel), len(wav) // hop)
        r = _ext.melcmp_host(a[None], np.asarray(mel, np.float32)[None], [F], num_mels=M, n_cep=n_cep_for(M), unit_db=_ext.melcmp_unit_db(hparams), alarm_db=alarm_db,
                             a_channels_first=True, b_channels_first=False, per_frame=False)
        frames.append(F)
        rows.append(np.concatenate((r['summary'][0], r['marks'][0].astype(np.float32))))
    return frames, np.stack(rows).astype(np.float32) if rows else np.zeros((0, 9), np.float32)


def score_device(wavs, mels, hparams, alarm_db=None, batch=32):
    """The same pairs on the device, `batch` at a time through one ReconstructionCheck."""
    import torch
    from datasets import audio
    hop, M = audio.get_hop_size(hparams), int(hparams.num_mels)
    frames = [min(len(m), len(w) // hop) for w, m in zip(wavs, mels)]
    out = np.zeros((len(wavs), 9), np.float32)
    if not wavs:
        return frames, out
    chk = ReconstructionCheck(hparams, min(batch, len(wavs)), max(len(w) for w in wavs), alarm_db=alarm_db)
    try:
        for lo in range(0, len(wavs), chk.rows):
            idx = list(range(lo, min(lo + chk.rows, len(wavs))))
            lens = [len(wavs[i]) for i in idx]
            x = np.zeros((len(idx), max(lens)), np.float32)
            c = np.zeros((len(idx), max(max(frames[i] for i in idx), 1), M), np.float32)
            for r, i in enumerate(idx):
                x[r, :lens[r]] = wavs[i]
                c[r, :frames[i]] = np.asarray(mels[i], np.float32)[:frames[i]]
            out[idx] = chk.score(torch.from_numpy(x).cuda(), lens, torch.from_numpy(c).cuda(), frames=[frames[i] for i in idx], c_channels_first=False)
    finally:
        chk.close()
    return frames, out


def read_pairs(map_path=None, wavs_dir=None, mels_dir=None):
    """(name, wav path, mel path) of every pair, and how many entries were skipped.  map_path: a map.txt written by synthesis, rows ``recording|mel|wav``
    (--wavs_dir runs) or ``mel|wav|speaker``: three columns, the mel (.npy) first or second and the wav right after it; any other row is skipped.
    Else: every wavenet-audio-<name>.wav of wavs_dir with <name>.npy (synthesis from mels) or mel-<name>.npy (from recordings) in mels_dir; a wav
    without either is skipped.  A path of a map row that does not exist as written is looked up by its file name next to the map."""
    pairs, skipped = [], 0
    if map_path is not None:
        base = os.path.dirname(os.path.abspath(map_path))
        with open(map_path, encoding='utf-8') as f:
            for line in f:
                if not line.strip():
                    continue
                cols = [s.strip() for s in line.strip().split('|')]
                at = 0 if cols[0].endswith('.npy') else 1
                if len(cols) != 3 or not cols[at].endswith('.npy') or not cols[at + 1].endswith('.wav'):
                    skipped += 1
                    continue
                mel, wav = [p if os.path.exists(p) else os.path.join(base, os.path.basename(p)) for p in cols[at:at + 2]]
                pairs.append((os.path.basename(wav)[:-4].replace('wavenet-audio-', '', 1), wav, mel))
    else:
        for n in sorted(os.listdir(wavs_dir)):
            if not (n.startswith('wavenet-audio-') and n.endswith('.wav')):
                continue
            name = n[len('wavenet-audio-'):-4]
            mel = next((c for c in ('{}.npy'.format(name), 'mel-{}.npy'.format(name)) if os.path.exists(os.path.join(mels_dir, c))), None)
            if mel is None:
                skipped += 1
                continue
            pairs.append((name, os.path.join(wavs_dir, n), os.path.join(mels_dir, mel)))
    return pairs, skipped


def main(argv=None):
    from datasets import audio
    from hparams import hparams as default_hparams
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--map', default=None, help='map.txt written by synthesis (recording|mel|wav or mel|wav|speaker rows)')
    ap.add_argument('--wavs', default=None, help='directory of wavenet-audio-<name>.wav (with --mels)')
    ap.add_argument('--mels', default=None, help='directory of mel-<name>.npy')
    ap.add_argument('--worst', type=int, default=10, help='how many of the worst utterances to list')
    ap.add_argument('--tsv', default=None, help='append the table here (the format of wavs/reconstruction.tsv)')
    ap.add_argument('--host', action='store_true', help='evaluate on the host (numpy analysis, the host hook): no GPU; the default is the device')
    ap.add_argument('--hparams', default='', help='comma separated name=value overrides')
    args = ap.parse_args(argv)
    if (args.map is None) == (args.wavs is None or args.mels is None):
        ap.error('give --map, or --wavs and --mels')
    hp = default_hparams.parse(args.hparams)
    pairs, skipped = read_pairs(args.map, args.wavs, args.mels)
    if skipped:
        print('skipped {} {} without a wav and mel pair'.format(skipped, 'row(s) of the map' if args.map else 'wav file(s)'))
    if not pairs:
        raise RuntimeError('no wav and mel pairs found')
    wavs = [audio.load_wav(w, sr=hp.sample_rate) for _, w, _ in pairs]        # the int16 file read back as float
    mels = [np.load(m) for _, _, m in pairs]
    lo, hi = (-hp.max_abs_value, hp.max_abs_value) if hp.symmetric_mels else (0, hp.max_abs_value)
    if hp.clip_for_wavenet:
        mels = [np.clip(m, lo, hi) for m in mels]
    frames, table = (score_host if args.host else score_device)(wavs, mels, hp)
    names = [n for n, _, _ in pairs]
    order = sorted(range(len(names)), key=lambda i: float(table[i, 4]))
    print('\t'.join(TSV_HEADER))
    for i in order:
        print(tsv_row(names[i], frames[i], table[i]))
    print(log_line(names, table))
    print('Worst utterances (l1c_db):')
    for i in order[::-1][:max(args.worst, 0)]:
        print('  {:8.3f}  frame {:5d} at {:8.3f} dB  {:4d} alarmed  {}'.format(float(table[i, 4]), int(table[i, 7]), float(table[i, 6]), int(table[i, 8]), names[i]))
    if args.tsv:
        append_tsv(args.tsv, names, frames, table)
    return names, frames, table


if __name__ == '__main__':
    main()
