"""Batch synthesis driver behind ``synthesize.py --model WaveNet | Tacotron-2`` (reference ``wavenet_vocoder/synthesize.py:69``
``wavenet_synthesize(args, hparams, checkpoint)``).  Inputs: every ``*.npy`` mel file of ``args.mels_dir`` (optionally one speaker id per
file in ``args.speaker_id``), or -- Tacotron-2 mode -- the ``text|mel|speaker`` rows of the Tacotron evaluation ``map.txt`` in that
directory.  Outputs, under ``wavenet_<output_dir>/``: ``wavs/wavenet-audio-<mel>.wav``, ``plots/``, and ``wavs/map.txt`` with one
``[text|]mel|wav|speaker`` row per utterance (the reference's format strings have one placeholder too few there, SURVEY appendix C-11:
its rows lose the last column; these keep it)."""
import os
from collections import namedtuple

import numpy as np
from tqdm import tqdm

from hparams import hparams_debug_string
from infolog import log
from wavenet_vocoder.synthesizer import Synthesizer
from wavenet_vocoder.train import get_checkpoint_state

Utterance = namedtuple('Utterance', 'text mel_path speaker')      # text None outside Tacotron-2 mode; speaker None without global conditioning


def _utterances(args):
    """The work list, in the order the reference walks it (sorted file names / map.txt row order)."""
    if args.model == 'Tacotron-2':
        with open(os.path.join(args.mels_dir, 'map.txt'), encoding='utf-8') as f:
            rows = [line.strip().split('|') for line in f if line.strip()]
        no_g = all(r[2] == '<no_g>' for r in rows)
        return [Utterance(r[0], r[1], None if no_g else r[2]) for r in rows]
    paths = sorted(os.path.join(args.mels_dir, name) for name in os.listdir(args.mels_dir) if name.rsplit('.', 1)[-1] == 'npy')
    speakers = [None] * len(paths)
    if args.speaker_id is not None:
        speakers = args.speaker_id.replace(' ', '').split(',')
        assert len(speakers) == len(paths), 'one speaker id per mel file'
    return [Utterance(None, p, s) for p, s in zip(paths, speakers)]


def run_synthesis(args, checkpoint_path, output_dir, hparams):
    plot_dir, wav_dir = os.path.join(output_dir, 'plots'), os.path.join(output_dir, 'wavs')
    log(hparams_debug_string())
    synth = Synthesizer()
    synth.load(checkpoint_path, hparams)
    work = _utterances(args)
    log('Starting synthesis! (this will take a while..)')
    for d in (plot_dir, wav_dir):
        os.makedirs(d, exist_ok=True)
    step = int(hparams.wavenet_synthesis_batch_size)
    with open(os.path.join(wav_dir, 'map.txt'), 'w') as index:
        for start in tqdm(range(0, len(work), step)):
            batch = work[start:start + step]
            mels = [np.load(u.mel_path) for u in batch]
            names = [os.path.basename(u.mel_path).replace('.npy', '') for u in batch]
            speakers = None if batch[0].speaker is None else [u.speaker for u in batch]
            wavs = synth.synthesize(mels, speakers, names, wav_dir, plot_dir)
            for u, wav in zip(batch, wavs):
                cols = ([] if u.text is None else [u.text]) + [u.mel_path, wav, '<no_g>' if u.speaker is None else u.speaker]
                index.write('|'.join(str(c) for c in cols) + '\n')
    log('synthesized audio waveforms at {}'.format(wav_dir))


def load_recordings(paths, hparams):
    """The recordings as float32 at hparams.sample_rate: audio.load_wav, which refuses another rate -- unless mi355_resample_input is on: then the off-rate
    files are converted first (datasets.wavenet_preprocessor.resample_off_rate: one handle per rate on the device) and the others are loaded as ever."""
    from datasets import audio
    converted = {}
    if getattr(hparams, 'mi355_resample_input', False):
        from datasets.wavenet_preprocessor import resample_off_rate
        converted = resample_off_rate(paths, hparams)
    return [converted[p] if p in converted else audio.load_wav(p, sr=hparams.sample_rate) for p in paths]


def analyse_wavs(paths, hparams, batch=32):
    """The conditioning mels of recordings, as preprocessing makes them (wavenet_preprocessor.py lines 71-76, 111: pre-emphasis, rescale to
    rescaling_max, melspectrogram) with every step on the device: wn_mel_peak gives max |preem_wav|, the gain rescaling_max / peak and the
    pre-emphasis are fused into wn_mel_run.  -> list of [frames, num_mels] float32 (frames = 1 + samples // hop)."""
    import torch
    from datasets import audio
    from wavenet_vocoder import _ext
    wavs = load_recordings(paths, hparams)
    for p, w in zip(paths, wavs):
        if w.size == 0:
            raise RuntimeError('empty recording: {}'.format(p))
    k = float(hparams.preemphasis) if hparams.preemphasize else 0.0
    analyzer = _ext.MelAnalyzer(hparams, min(batch, len(wavs)), max(len(w) for w in wavs), preemphasis=k)
    mels = [None] * len(wavs)
    order = sorted(range(len(wavs)), key=lambda i: len(wavs[i]))
    try:
        for lo in range(0, len(order), analyzer.max_batch):
            idx = order[lo:lo + analyzer.max_batch]
            lens = [len(wavs[i]) for i in idx]
            host = np.zeros((len(idx), max(lens)), dtype=np.float32)
            for r, i in enumerate(idx):
                host[r, :lens[r]] = wavs[i]
            dev = torch.from_numpy(host).cuda()
            gain = None
            if hparams.rescale:
                gain = float(hparams.rescaling_max) / analyzer.peak(dev, lens).clamp_min(1e-30)
            c = analyzer.run(dev, lens, gain=gain, channels_first=True)          # [B, num_mels, F]: the layout the engine takes as c
            c = c.transpose(1, 2).cpu().numpy()
            for r, i in enumerate(idx):
                mels[i] = np.ascontiguousarray(c[r, :1 + lens[r] // analyzer.hop])
    finally:
        analyzer.close()
    return mels


def pitch_references(paths, hparams):
    """The recordings as the pitch check takes them (mi355_pitch_check): pre-emphasised as preprocessing does it, so that they stand beside the
    model-domain output; the estimator is scale-invariant, so the rescale is left out."""
    from datasets import audio
    return [audio.preemphasis(w, hparams.preemphasis, hparams.preemphasize).astype(np.float32) for w in load_recordings(paths, hparams)]


def run_wav_synthesis(args, checkpoint_path, output_dir, hparams):
    """--wavs_dir: analysis then synthesis.  Writes wavs/wavenet-audio-<basename>.wav (mel_frames * hop samples), the analysed mel next to
    it as wavs/mel-<basename>.npy, and wavs/map.txt rows ``recording|mel|wav``; with mi355_pitch_check also one row per utterance in wavs/pitch.tsv."""
    plot_dir, wav_dir = os.path.join(output_dir, 'plots'), os.path.join(output_dir, 'wavs')
    log(hparams_debug_string())
    if hparams.gin_channels > 0:
        raise RuntimeError('--wavs_dir: a globally conditioned WaveNet needs speaker ids; analyse with wavenet_preprocess.py and use --mels_dir --speaker_id')
    paths = sorted(os.path.join(args.wavs_dir, n) for n in os.listdir(args.wavs_dir) if n.endswith('.wav'))
    if not paths:
        raise RuntimeError('no *.wav in {}'.format(args.wavs_dir))
    synth = Synthesizer()
    synth.load(checkpoint_path, hparams)
    for d in (plot_dir, wav_dir):
        os.makedirs(d, exist_ok=True)
    step = int(hparams.wavenet_synthesis_batch_size)
    live_ms = float(getattr(hparams, 'mi355_synthesis_live_chunk_ms', 0))
    if live_ms > 0:
        return run_live_wav_synthesis(synth, paths, wav_dir, hparams, live_ms)
    with open(os.path.join(wav_dir, 'map.txt'), 'w') as index:
        for start in tqdm(range(0, len(paths), step)):
            batch = paths[start:start + step]
            names = [os.path.basename(p)[:-len('.wav')] for p in batch]
            mels = analyse_wavs(batch, hparams)
            mel_paths = [os.path.join(wav_dir, 'mel-{}.npy'.format(n)) for n in names]
            for mp, mel in zip(mel_paths, mels):
                np.save(mp, mel, allow_pickle=False)
            if bool(getattr(hparams, 'mi355_pitch_check', False)):
                synth.pitch_references = pitch_references(batch, hparams)
            wavs = synth.synthesize(mels, None, names, wav_dir, plot_dir)
            for p, mp, wav in zip(batch, mel_paths, wavs):
                index.write('|'.join([p, mp, wav]) + '\n')
    log('synthesized audio waveforms at {}'.format(wav_dir))


def run_live_wav_synthesis(synth, paths, wav_dir, hparams, chunk_ms):
    """mi355_synthesis_live_chunk_ms > 0: the recordings chunk by chunk through wavenet_vocoder.live.LiveVocoder -- never a whole recording on the device, the
    analysis and the generation push by push, each wav growing as it is generated (int16 from the device output stage).  The rescale gain comes from a first
    chunked pass over the file (live's --gain peak), so mel-<basename>.npy holds the bytes analyse_wavs gives.  Same file names and map.txt rows as the
    whole-recording route; silence is not trimmed and no plots are made."""
    from datasets.audio import get_hop_size
    from wavenet_vocoder import live
    hop = get_hop_size(hparams)
    chunk = max(1, int(round(hparams.sample_rate * chunk_ms / 1000.0)))
    rows = max(1, min(len(paths), int(hparams.wavenet_synthesis_batch_size), 32))
    synth._ensure_capacity(rows, (chunk // hop + 12) * hop)      # a push generates the frames of one chunk, and at the end those the look-ahead held back
    names = [os.path.basename(p)[:-len('.wav')] for p in paths]
    outs = [os.path.join(wav_dir, 'wavenet-audio-{}.wav'.format(n)) for n in names]
    mel_paths = [os.path.join(wav_dir, 'mel-{}.npy'.format(n)) for n in names]
    live.vocode_files(synth.model, paths, outs, chunk, gain='peak', mel_paths=mel_paths, rows=rows)
    with open(os.path.join(wav_dir, 'map.txt'), 'w') as index:
        for p, mp, wav in zip(paths, mel_paths, outs):
            index.write('|'.join([p, mp, wav]) + '\n')
    log('synthesized audio waveforms at {}'.format(wav_dir))


def wavenet_synthesize(args, hparams, checkpoint):
    checkpoint_path = get_checkpoint_state(checkpoint)
    if checkpoint_path is None or not (os.path.exists(checkpoint_path) or os.path.exists(checkpoint_path + '.index')):
        raise RuntimeError('Failed to load checkpoint at {}'.format(checkpoint))
    log('loaded model at {}'.format(checkpoint_path))
    if getattr(args, 'wavs_dir', None):
        return run_wav_synthesis(args, checkpoint_path, 'wavenet_' + args.output_dir, hparams)
    run_synthesis(args, checkpoint_path, 'wavenet_' + args.output_dir, hparams)
