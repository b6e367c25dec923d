"""WaveNet dataset preprocessing (reference datasets/wavenet_preprocessor.py: build_from_path / _process_utterance, lines 58-154): a folder
of wav files -> audio/audio-<name>.npy (the network's target, encoded for hparams.input_type), mels/mel-<name>.npy ([frames, num_mels]
float32) and the rows of map.txt.

Split in two so that at most one process opens the GPU.  The host steps of an utterance -- load, silence trim, pre-emphasis, rescale and
range check, mu-law encoding with its own silence trim -- run in worker processes (spawned: they import numpy / scipy only and never touch
the device).  The parent then takes the mel-spectrograms of all pre-emphasised signals from ONE _ext.MelAnalyzer in batches of neighbouring
lengths (hparams.mi355_device_mel; False: datasets.audio.melspectrogram in numpy float64, utterance by utterance) and finishes each
utterance: length clip, right padding with the encoding's silence value, truncation to mel_frames * hop, the two files, the row.

hparams.mi355_resample_input (default off: a file at another rate than sample_rate is load_wav's error) lets the folder hold wavs of any rate: the
parent reads the off-rate files, converts them rate by rate (resample_off_rate: one _ext.Resampler per rate on the GPU, csrc/wn_resample.hip; the host
loop with the same bits where there is none) and hands the float32 signal to the worker in place of the path's samples.  Still one process on the GPU."""
import os
from concurrent.futures import ProcessPoolExecutor
from multiprocessing import get_context

import numpy as np

from datasets import audio
from wavenet_vocoder.util import is_mulaw, is_mulaw_quantize, mulaw, mulaw_quantize

DEVICE_BATCH = 32


def _host_steps(wav_path, hparams, wav=None):
    """Reference _process_utterance lines 58-108.  -> None (file missing) or (encoded audio, float32 pre-emphasised signal for the mel
    analysis, silence value, audio dtype name, length of the signal the padding is computed from).  wav: the float32 signal at
    hparams.sample_rate where the parent has already read and converted the file (mi355_resample_input); None: load it here."""
    if wav is None:
        try:
            wav = audio.load_wav(wav_path, sr=hparams.sample_rate)
        except FileNotFoundError:
            print('skipped (vanished since the folder was listed): {}'.format(wav_path))
            return None
    if hparams.trim_silence:
        wav = audio.trim_silence(wav, hparams)
    if wav.size == 0:
        raise RuntimeError('nothing but silence in: {}'.format(wav_path))
    preem_wav = audio.preemphasis(wav, hparams.preemphasis, hparams.preemphasize)
    if hparams.rescale:
        wav = wav / np.abs(wav).max() * hparams.rescaling_max
        preem_wav = preem_wav / np.abs(preem_wav).max() * hparams.rescaling_max
        if (wav > 1.).any() or (wav < -1.).any() or (preem_wav > 1.).any() or (preem_wav < -1.).any():
            raise RuntimeError('{}: samples outside [-1, 1] after rescaling to rescaling_max = {}'.format(wav_path, hparams.rescaling_max))
    if is_mulaw_quantize(hparams.input_type):
        out = mulaw_quantize(wav, hparams.quantize_channels)                      # [0, quantize_channels)
        start, end = audio.start_and_end_indices(out, hparams.silence_threshold)
        wav, preem_wav, out = wav[start:end], preem_wav[start:end], out[start:end]
        constant_values, out_dtype = mulaw_quantize(0, hparams.quantize_channels), 'int16'
    elif is_mulaw(hparams.input_type):
        out = mulaw(wav, hparams.quantize_channels)                               # [-1, 1]
        constant_values, out_dtype = mulaw(0., hparams.quantize_channels), 'float32'
    else:
        out, constant_values, out_dtype = wav, 0., 'float32'
    return np.asarray(out), np.asarray(preem_wav), constant_values, out_dtype, len(wav)


def _finish(name, host, mel, mel_dir, wav_dir, hparams):
    """Reference _process_utterance lines 110-154; mel: float32 [num_mels, frames]."""
    out, _, constant_values, out_dtype, n = host
    hop = audio.get_hop_size(hparams)
    mel_frames = mel.shape[1]
    if mel_frames > hparams.max_mel_frames and hparams.clip_mels_length:
        return None
    _, r_pad = audio.librosa_pad_lr(np.empty(n), hparams.n_fft, hop)
    out = np.pad(out, (0, r_pad), mode='constant', constant_values=constant_values)
    assert len(out) >= mel_frames * hop
    out = out[:mel_frames * hop]                    # a multiple of hop: the upsampling network maps frames to samples exactly
    time_steps = len(out)
    audio_filename = os.path.join(wav_dir, 'audio-{}.npy'.format(name))
    mel_filename = os.path.join(mel_dir, 'mel-{}.npy'.format(name))
    np.save(audio_filename, out.astype(out_dtype), allow_pickle=False)
    np.save(mel_filename, np.ascontiguousarray(mel.T, dtype=np.float32), allow_pickle=False)
    if hparams.gin_channels > 0:
        raise RuntimeError('gin_channels > 0: global conditions need a rule that maps a file name to its speaker id, and this preprocessor has none '
                           '(add one in datasets/wavenet_preprocessor.py:_finish; the map.txt column is <no_g> otherwise)')
    return (audio_filename, mel_filename, mel_filename, '<no_g>', time_steps, mel_frames)


def _mels(signals, hparams):
    """float32 [num_mels, frames] per signal: the device (mi355_device_mel) or numpy float64."""
    if not getattr(hparams, 'mi355_device_mel', False):
        return [audio.melspectrogram(np.asarray(s, dtype=np.float64), hparams).astype(np.float32) for s in signals]
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError('mi355_device_mel=True needs an MI355X (the HIP library is the only device path); --hparams mi355_device_mel=False analyses in numpy')
    from wavenet_vocoder import _ext
    analyzer = _ext.MelAnalyzer(hparams, min(DEVICE_BATCH, len(signals)), max(len(s) for s in signals))
    try:
        return audio.melspectrogram_device(signals, hparams, analyzer=analyzer)
    finally:
        analyzer.close()


def _wav_rate(path):
    """the sample rate in the file's header (memory-mapped: the samples are not read); None for a file that has vanished"""
    from scipy.io import wavfile
    try:
        return int(wavfile.read(path, mmap=True)[0])
    except FileNotFoundError:
        return None


def resample_off_rate(paths, hparams):
    """mi355_resample_input: {path: float32 signal at hparams.sample_rate} for the files of `paths` at another rate, read here and converted rate by rate
    (audio.resample_signals: one handle per rate on the GPU, the host loop with the same bits without one).  Files at sample_rate are not in the result:
    they never pass through the resampler."""
    by_rate = {}
    for p in paths:
        rate = _wav_rate(p)
        if rate is not None and rate != int(hparams.sample_rate):
            by_rate.setdefault(rate, []).append(p)
    converted = {}
    for rate in sorted(by_rate):
        signals = [audio.read_wav(p)[1] for p in by_rate[rate]]
        for p, y in zip(by_rate[rate], audio.resample_signals(signals, rate, int(hparams.sample_rate))):
            converted[p] = y
    return converted


def build_from_path(hparams, input_dir, mel_dir, wav_dir, n_jobs=12, tqdm=lambda x: x):
    """Preprocess every *.wav of input_dir (sorted by name: two runs write the same map.txt).  Returns the map.txt rows
    (audio_filename, mel_filename, mel_filename, '<no_g>', time_steps, mel_frames) of the utterances that were kept."""
    if getattr(hparams, 'use_lws', False):
        raise NotImplementedError('use_lws: the lws package is not available')
    names = sorted(f for f in os.listdir(input_dir) if f.endswith('.wav'))
    paths = [os.path.join(input_dir, f) for f in names]
    converted = resample_off_rate(paths, hparams) if getattr(hparams, 'mi355_resample_input', False) else {}      # (the parent: still one process on the GPU)
    if n_jobs and n_jobs > 1 and len(paths) > 1:
        with ProcessPoolExecutor(max_workers=min(n_jobs, len(paths)), mp_context=get_context('spawn')) as executor:
            futures = [executor.submit(_host_steps, p, hparams, converted.get(p)) for p in paths]
            hosts = [f.result() for f in tqdm(futures)]
    else:
        hosts = [_host_steps(p, hparams, converted.get(p)) for p in tqdm(paths)]
    kept = [(f[:-len('.wav')], h) for f, h in zip(names, hosts) if h is not None]
    if not kept:
        return []
    mels = _mels([h[1].astype(np.float32) if getattr(hparams, 'mi355_device_mel', False) else h[1] for _, h in kept], hparams)
    rows = [_finish(name, h, mel, mel_dir, wav_dir, hparams) for (name, h), mel in zip(kept, mels)]
    return [r for r in rows if r is not None]
