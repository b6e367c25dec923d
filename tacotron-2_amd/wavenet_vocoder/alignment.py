"""Alignment check: a generated utterance against a recording of ANOTHER length and timing, per utterance.

    python -m wavenet_vocoder.alignment --generated DIR --reference DIR [--tsv FILE] [--band N] [--host] [--hparams ...]

What the reconstruction and pitch checks cannot score.  Both need frame-aligned signals; the output of ``synthesize.py --mels_dir`` on PREDICTED mels has the
timing the predictor gave it.  Here both signals are analysed as preprocessing analyses a recording (csrc/wn_mel.hip), their mel cepstra are aligned by dynamic
time warping on the device (csrc/wn_align.hip) and the mel-cepstral distortion is averaged along the path (MCD-DTW, dB); both are tracked by the pitch check's
estimator (csrc/wn_pitch.hip), the generated F0 track is warped onto the recording's frames with the path's frame map, and the two tracks are compared as the
pitch check compares them: F0 RMSE, voicing error and gross pitch error along the same path.  Both signals must be in one domain: the drivers pre-emphasise the
recording as preprocessing does, so that it stands beside the model-domain output.  What a good mcd_dtw is for a trained model is not known here: nobody has one."""
import argparse
import os

import numpy as np

# the aligner's summary with a = the recording and b = the generated signal, then columns 3 ... 8 of the pitch comparison over the recording's frames
COLUMNS = ('frames_ref', 'frames_gen', 'n_path', 'total', 'mcd_dtw', 'stretch', 'deviation', 'both', 'vuv_error', 'gpe', 'f0_rmse_cents', 'f0_bias_cents', 'f0_fine_rmse_cents')
TSV_HEADER = ('name',) + COLUMNS
MAX_FRAMES = 4096          # per signal: the aligner's reserve limit (about 51 s at a hop of 12.5 ms)


def _n_cep(num_mels):
    from wavenet_vocoder.reconstruction import n_cep_for
    return n_cep_for(num_mels)


def _band(hparams, band):
    return int(getattr(hparams, 'mi355_alignment_band', 0)) if band is None else int(band)


class AlignmentCheck(object):
    """One MelAnalyzer, one Aligner and one PitchTracker for up to `rows` pairs of signals of up to `max_samples` samples each: geometry, unit_db and the
    pre-emphasis of the analysis from the hparams as the reconstruction check takes them, the band from mi355_alignment_band unless given."""

    def __init__(self, hparams, rows, max_samples, band=None):
        from datasets.audio import get_hop_size
        from wavenet_vocoder import _ext
        self.hop, self.num_mels = int(get_hop_size(hparams)), int(hparams.num_mels)
        self.rows, self.max_samples = int(rows), int(max_samples)
        self.max_frames = 1 + self.max_samples // self.hop
        self.band = _band(hparams, band)
        pre = float(hparams.preemphasis) if hparams.preemphasize else 0.0
        self.aligner = _ext.Aligner(self.num_mels, self.rows, self.max_frames, self.max_frames, n_cep=_n_cep(self.num_mels), unit_db=_ext.melcmp_unit_db(hparams), band=self.band)
        self.analyzer = _ext.MelAnalyzer(hparams, self.rows, self.max_samples, preemphasis=pre)
        self.tracker = _ext.PitchTracker(hparams, self.rows, self.max_samples)

    def score(self, generated, gen_lengths, reference, ref_lengths, maps=False):
        """generated, reference: device float [B, ld] each (ld may differ), both in one domain; row b holds gen_lengths[b] resp. ref_lengths[b] samples.
        Analysis, alignment, both F0 tracks, the warp (a gather by map_ab) and the comparison run on the device; ONE copy brings the result to the host:
        float32 [B, 13], columns COLUMNS.  maps: also the device tensors (map_ab over the recording's frames, f0_ref, the warped f0_gen)."""
        import torch
        gl, rl = [int(n) for n in gen_lengths], [int(n) for n in ref_lengths]
        fg, fr = [1 + n // self.hop for n in gl], [1 + n // self.hop for n in rl]
        generated, reference = generated.float().contiguous(), reference.float().contiguous()
        mel_ref = self.analyzer.run(reference, rl, channels_first=True)
        mel_gen = self.analyzer.run(generated, gl, channels_first=True)
        out = self.aligner.run(mel_ref, mel_gen, fr, fg, want=('map_ab',))
        f0_ref = self.tracker.run(reference, rl)[0]
        f0_gen = self.tracker.run(generated, gl)[0]
        idx = out['map_ab'].clamp(0, int(f0_gen.shape[1]) - 1).to(torch.int64)          # (cells beyond a row's frames are not compared)
        warped = torch.gather(f0_gen, 1, idx).contiguous()
        table = self.tracker.compare(f0_ref, warped, fr)
        res = torch.cat((out['summary'], table[:, 3:]), dim=1).cpu().numpy()
        return (res, out['map_ab'], f0_ref, warped) if maps else res

    def close(self):
        for st in (self.aligner, self.analyzer, self.tracker):
            st.close()


def dtw(cost, band=0):
    """Dynamic time warping of a cost matrix [Fa, Fb] in float64 on the host, numpy only, with the recurrence, band and tie order of csrc/wn_align.h:
    -> (total, path int64 [n, 2] in forward order).  For users without a device; seconds per utterance."""
    cost = np.asarray(cost, np.float64)
    Fa, Fb = cost.shape
    W = int(band) * max(Fa, Fb)
    dm = np.full((Fa, Fb), np.inf)
    dirs = np.full((Fa, Fb), 3, np.int8)
    for i in range(Fa):
        lo, hi = (0, Fb - 1) if band == 0 else (max(0, -((W - i * Fb) // Fa)), min(Fb - 1, (i * Fb + W) // Fa))
        up = dm[i - 1] if i > 0 else None
        row, left = dm[i], np.inf
        for j in range(lo, hi + 1):
            if i == 0 and j == 0:
                row[0] = left = cost[0, 0]
                continue
            best, w = np.inf, 3
            if i > 0 and j > 0 and up[j - 1] < np.inf:
                best, w = up[j - 1], 0
            if i > 0 and up[j] < best:
                best, w = up[j], 1
            if j > lo and left < best:
                best, w = left, 2
            if w != 3:
                row[j] = cost[i, j] + best
                dirs[i, j] = w
            left = row[j]
    i, j, rev = Fa - 1, Fb - 1, []
    while i > 0 or j > 0:
        rev.append((i, j))
        w = 2 if i == 0 else 1 if j == 0 else 0 if dirs[i, j] == 3 else dirs[i, j]
        i, j = i - (w != 2), j - (w != 1)
    rev.append((0, 0))
    return float(dm[-1, -1]), np.array(rev[::-1], np.int64)


def _host_mel(wav, hparams):
    from datasets import audio
    x = audio.preemphasis(np.asarray(wav, dtype=np.float64), hparams.preemphasis, hparams.preemphasize)
    return audio.melspectrogram(x, hparams).astype(np.float32)                    # [M, 1 + n // hop]


def score_host(generated, reference, hparams, band=None):
    """The host evaluation of the same check (numpy analysis in float64, the hooks of csrc/wn_align.h and csrc/wn_pitch.h for the rest): no GPU.  generated,
    reference: lists of 1-D float arrays of any lengths.  -> float32 [N, 13]."""
    from wavenet_vocoder import _ext
    M = int(hparams.num_mels)
    geo = _ext.pitch_geometry(hparams)
    rows = []
    for g, r in zip(generated, reference):
        g, r = np.asarray(g, np.float32), np.asarray(r, np.float32)
        mg, mr = _host_mel(g, hparams), _host_mel(r, hparams)
        fg, fr = mg.shape[1], mr.shape[1]
        al = _ext.align_host(mr[None], mg[None], [fr], [fg], num_mels=M, n_cep=_n_cep(M), unit_db=_ext.melcmp_unit_db(hparams), band=_band(hparams, band))
        f0g = _ext.pitch_host(geo, g[None], [len(g)], frames=fg)['f0']
        f0r = _ext.pitch_host(geo, r[None], [len(r)], frames=fr)['f0']
        warped = np.ascontiguousarray(f0g[:, al['map_ab'][0, :fr]])
        rows.append(np.concatenate((al['summary'][0], _ext.pitch_compare_host(f0r, warped, [fr])[0, 3:])))
    return np.stack(rows).astype(np.float32) if rows else np.zeros((0, len(COLUMNS)), np.float32)


def score_device(generated, reference, hparams, band=None, batch=8):
    """The same pairs on the device, `batch` at a time through one AlignmentCheck."""
    import torch
    out = np.zeros((len(generated), len(COLUMNS)), np.float32)
    if not generated:
        return out
    chk = AlignmentCheck(hparams, min(batch, len(generated)), max(max(len(g), len(r)) for g, r in zip(generated, reference)), band=band)
    try:
        for lo in range(0, len(generated), chk.rows):
            idx = list(range(lo, min(lo + chk.rows, len(generated))))
            gl, rl = [len(generated[i]) for i in idx], [len(reference[i]) for i in idx]
            g, r = np.zeros((len(idx), max(max(gl), 1)), np.float32), np.zeros((len(idx), max(max(rl), 1)), np.float32)
            for k, i in enumerate(idx):
                g[k, :gl[k]] = np.asarray(generated[i], np.float32)
                r[k, :rl[k]] = np.asarray(reference[i], np.float32)
            out[idx] = chk.score(torch.from_numpy(g).cuda(), gl, torch.from_numpy(r).cuda(), rl)
    finally:
        chk.close()
    return out


def tsv_row(name, row):
    vals = [str(int(v)) for v in row[:3]] + ['{:.4f}'.format(float(v)) for v in row[3:7]] + [str(int(row[7]))] + ['{:.4f}'.format(float(v)) for v in row[8:10]] + [
        '{:.2f}'.format(float(v)) for v in row[10:13]]
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


def log_line(names, table):
    """The batch means, and the worst utterance by mcd_dtw."""
    table = np.asarray(table, dtype=np.float64).reshape(-1, len(COLUMNS))
    w = int(np.argmax(table[:, 4]))
    return ('Alignment check: {} utterance(s), mean MCD-DTW {:.2f} dB, stretch share {:.3f}, F0 RMSE {:.1f} cents, V/UV error {:.3f}, gross pitch error {:.3f}; worst {} '
            '(MCD-DTW {:.2f} dB over a path of {} cells)').format(len(names), table[:, 4].mean(), table[:, 5].mean(), table[:, 10].mean(), table[:, 8].mean(), table[:, 9].mean(),
                                                                   names[w], table[w, 4], int(table[w, 2]))


def reference_for(reference_dir, basename):
    """The recording an utterance is scored against: <reference_dir>/<basename>.wav, else the same without a leading ``mel-`` (the names preprocessing and
    --wavs_dir give their mel files); None when there is neither."""
    for n in (basename, basename[len('mel-'):] if basename.startswith('mel-') else None):
        if n and os.path.exists(os.path.join(reference_dir, n + '.wav')):
            return os.path.join(reference_dir, n + '.wav')
    return None


def main(argv=None):
    from datasets import audio
    import hparams as H
    from wavenet_vocoder.pitch import read_pairs
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--generated', required=True, help='directory of generated wavs')
    ap.add_argument('--reference', required=True, help='directory of recordings of equal names (any lengths)')
    ap.add_argument('--tsv', default=None, help='append the table here (the format of wavs/alignment.tsv)')
    ap.add_argument('--band', type=int, default=None, help='the band of the alignment (default: mi355_alignment_band)')
    ap.add_argument('--host', action='store_true', help='evaluate on the host (numpy analysis, the hooks: the same arithmetic): no GPU; the default is the device')
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
    table = (score_host if args.host else score_device)(gen, ref, hp, band=args.band)
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
