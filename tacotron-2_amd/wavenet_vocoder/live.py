"""Live vocoding: recordings that arrive chunk by chunk are analysed and generated push by push, every stage on the device with a small per-row state --
[input Resampler ->] MelStream -> SlotSession [-> stream denoiser -> output stage -> output resampler].  Host-side bookkeeping only: LiveVocoder chains the
existing pushes and adds no kernel.  A row's frames are those of the whole recording (MelStream is bit-identical to MelAnalyzer.run), so its samples are those
of a SlotSession fed the whole analysed mel in the same slot with the same seed.

    python -m wavenet_vocoder.live --checkpoint DIR --input a.wav [b.wav ...] --output_dir OUT --chunk_ms 100 [--gain 1 | peak]

reads the files chunk by chunk, holds at most one push per row on the device and writes each output wav as it grows.  Silence is not trimmed (that needs the
whole utterance's maximum).  The audio lags the recording by MelStream.lag_samples plus the upsampler's look-ahead frames (LiveVocoder.lag_samples)."""
import argparse
import os
import sys
from collections import namedtuple

import numpy as np

LiveChunk = namedtuple('LiveChunk', 'frames result')      # frames: the row's new mel frames [num_mels, n_out] as analysed; result: what SlotSession.push returned for the row


def conditioning_range(hp):
    return (-float(hp.max_abs_value), float(hp.max_abs_value)) if hp.symmetric_mels else (0.0, float(hp.max_abs_value))


def condition(hp, mel):
    """analysed mel frames (torch, any shape) -> what the model takes as c: Synthesizer.synthesize's clip_for_wavenet and normalize_for_wavenet"""
    lo, hi = conditioning_range(hp)
    if hp.clip_for_wavenet:
        mel = mel.clamp(lo, hi)
    if hp.normalize_for_wavenet:
        mel = (mel - lo) / (hi - lo)
    return mel


def peak_gain(hp, peak, device='cpu'):
    """the rescale gain of preprocessing, rescaling_max / max(peak, 1e-30), by the very float32 expression analyse_wavs evaluates (torch divides a scalar by a
    tensor as reciprocal times scalar), on `device`: the bits of its gain"""
    import torch
    g = float(hp.rescaling_max) / torch.tensor([float(peak)], dtype=torch.float32, device=device).clamp_min(1e-30)
    return float(g[0])


def chunked_peak(chunks, k):
    """max |x[s] - k x[s - 1]| over a recording given as float32 chunks, in the float32 operations of wn_mel_peak (x[-1] = 0)"""
    k, last, peak = np.float32(k), np.float32(0.0), np.float32(0.0)
    for x in chunks:
        x = np.asarray(x, np.float32)
        if x.size == 0:
            continue
        prev = np.concatenate([[last], x[:-1]]).astype(np.float32)
        peak = max(peak, np.max(np.abs(x - k * prev)))
        last = x[-1]
    return float(peak)


class LiveVocoder(object):
    """rows recordings at a time through one MelStream and one slot session of `model` (model.slots(rows), or model.wide_slots(rows) above 32 rows; the engine
    must have been built for `rows` and for the samples of one push).  max_push: most samples per row in one push(), at the rate they arrive at.
    input_sample_rate: that rate when it is not hparams.sample_rate (an input Resampler converts first).  post / denoise / resample: an output stage, a stream
    denoiser and an output resampler of >= rows rows (WaveNet.output_stage / stream_denoiser / output_resampler), handed to SlotSession.push as they are and
    closed with the vocoder."""

    def __init__(self, model, rows, max_push, preemphasis=None, input_sample_rate=None, post=None, post_output='pcm', denoise=None, denoise_strength=None, resample=None,
                 steps_per_graph=None):
        hp = model._hparams
        self.model, self.hp, self.rows, self.max_push = model, hp, int(rows), int(max_push)
        self.input_resampler = None
        mel_push = self.max_push
        if input_sample_rate is not None and int(input_sample_rate) != int(hp.sample_rate):
            from wavenet_vocoder import _ext
            self.input_resampler = _ext.Resampler(int(input_sample_rate), int(hp.sample_rate), self.rows, self.max_push)
            mel_push = self.input_resampler.num_out(self.max_push + 2 * self.input_resampler.W) + 1      # what one push of the resampler can emit
        self.mel = model.mel_stream(self.rows, mel_push, preemphasis)
        self.session = (model.wide_slots if self.rows > 32 else model.slots)(self.rows, steps_per_graph=steps_per_graph)
        self.post, self.post_output, self.denoise, self.denoise_strength, self.resample = post, post_output, denoise, denoise_strength, resample
        self._open, self._restart, self._gain = [False] * self.rows, [False] * self.rows, [1.0] * self.rows
        self.frames_in = [0] * self.rows      # mel frames handed to the session per open row
        self.closed = False

    @property
    def lag_samples(self):
        """samples by which the audio trails the recording: the analysis window's right half, then the upsampler's look-ahead frames"""
        return self.mel.lag_samples + self.session.lookahead[1] * self.mel.hop

    def open(self, row, seed=None, g=None, gain=1.0):
        """start a recording in an idle row (live with the next push).  gain: the factor on the pre-emphasised signal, latched for the recording (1: the live
        case; peak_gain(...) reproduces preprocessing's rescale).  seed, g: as SlotSession.open."""
        if self._open[row]:
            raise ValueError('LiveVocoder.open: row %d is busy' % row)
        self.session.open(row, g=g, seed=seed)
        self._open[row], self._restart[row], self._gain[row], self.frames_in[row] = True, True, float(gain), 0

    def push(self, chunks, n=None, final=None):
        """chunks: float32 [rows, pitch] (torch on the device, or numpy), n: samples per row (None: the whole pitch for open rows), final: flags per row (None:
        none).  Rows that are not open must have n = 0.  Returns {row: LiveChunk} for every open row that was given samples or ended: its new mel frames and the
        session's result (samples, with post / denoise / resample the playable chunk last)."""
        import torch
        if self.closed:
            raise RuntimeError('LiveVocoder: closed')
        if isinstance(chunks, np.ndarray):
            chunks = torch.from_numpy(np.ascontiguousarray(chunks, dtype=np.float32)).to(self.model.device)
        B = self.rows
        n = [int(chunks.shape[1]) if self._open[b] else 0 for b in range(B)] if n is None else [int(v) for v in n]
        final = [False] * B if final is None else [bool(v) for v in final]
        if len(n) != B or len(final) != B or int(chunks.shape[0]) != B:
            raise ValueError('LiveVocoder.push: one row of chunks, one n and one final flag per row (%d rows)' % B)
        for b in range(B):
            if (n[b] > 0 or final[b]) and not self._open[b]:
                raise ValueError('LiveVocoder.push: row %d is idle (open it first)' % b)
        named = [b for b in range(B) if n[b] > 0 or final[b]]
        restart = [int(self._restart[b] and b in named) for b in range(B)]
        x = chunks
        if self.input_resampler is not None:
            x, n = self.input_resampler.push(x, n=n, restart=restart, final=[int(f) for f in final])
        mel, n_out = self.mel.push(x, n=n, restart=restart, final=[int(f) for f in final], gain=self._gain, channels_first=True)
        c = condition(self.hp, mel)
        items = {b: (c[b, :, :n_out[b]], final[b]) for b in named}
        res = self.session.push(items, post=self.post, post_output=self.post_output, denoise=self.denoise, denoise_strength=self.denoise_strength, resample=self.resample)
        out = {}
        for b in named:
            self._restart[b] = False
            self.frames_in[b] += n_out[b]
            out[b] = LiveChunk(mel[b, :, :n_out[b]], res[b])
            if final[b]:
                self._open[b] = False
        return out

    def check(self):
        self.session.check()

    def close(self):
        if self.closed:
            return
        self.closed = True
        self.session.close()
        for h in (self.mel, self.input_resampler, self.post, self.denoise, self.resample):
            if h is not None:
                h.close()


def samples_of(result):
    """the model-domain samples of a SlotSession.push result (its first element when a playable chunk follows)"""
    return result[0] if isinstance(result, tuple) else result


class WavReader(object):
    """a wav file read chunk by chunk as float32 in [-1, 1) (int16 / int32 / float PCM through scipy's memory map: nothing but the chunk is held)"""

    def __init__(self, path):
        from scipy.io import wavfile
        self.rate, data = wavfile.read(path, mmap=True)
        self.data = data[:, 0] if data.ndim > 1 else data
        self.pos = 0

    def __len__(self):
        return int(self.data.shape[0])

    def rewind(self):
        self.pos = 0

    def read(self, n):
        x = np.asarray(self.data[self.pos:self.pos + n])
        self.pos += len(x)
        if x.dtype == np.int16:
            return x.astype(np.float32) / 32768.0
        if x.dtype == np.int32:
            return (x.astype(np.float64) / 2147483648.0).astype(np.float32)
        return x.astype(np.float32)

    def chunks(self, n):
        """the rest of the file, n samples at a time"""
        while not self.done:
            yield self.read(n)

    @property
    def done(self):
        return self.pos >= len(self)


class GrowingWav(object):
    """a 16-bit mono wav written as it grows: the header's sizes are brought up to date after every append, so the file is playable at any time"""

    def __init__(self, path, rate):
        import wave
        self.w = wave.open(path, 'wb')
        self.w.setnchannels(1); self.w.setsampwidth(2); self.w.setframerate(int(rate))

    def append(self, pcm):
        self.w.writeframes(np.ascontiguousarray(pcm, dtype='<i2').tobytes())      # (writeframes patches the header)
        self.w._file.flush()

    def close(self):
        self.w.close()


def vocode_files(model, paths, out_paths, chunk_samples, gain='1', mel_paths=None, rows=None, seed_base=None, progress=None):
    """The recordings `paths` (all at hparams.sample_rate, or all at one other rate: an input Resampler converts) through one LiveVocoder of
    rows = min(len(paths), rows or 32) rows, chunk_samples per push and row; each out_paths[i] grows as its recording is generated (int16 through the model's
    output stage on the device).  gain: '1', or 'peak' (a first chunked host pass over the file gives max |preem|, and the rescale gain of preprocessing
    follows).  mel_paths: where to save each recording's analysed mel [frames, num_mels] (None: nowhere).  Returns the frames of every recording."""
    import torch
    hp = model._hparams
    readers = [WavReader(p) for p in paths]
    rates = sorted(set(r.rate for r in readers))
    if len(rates) != 1:
        raise RuntimeError('the recordings must share one sample rate (got %r)' % rates)
    k = float(hp.preemphasis) if hp.preemphasize else 0.0
    B = min(len(paths), int(rows or 32))
    post = model.output_stage(B)
    voc = LiveVocoder(model, B, chunk_samples, input_sample_rate=rates[0], post=post, post_output='pcm')
    owner, waiting = [None] * B, list(range(len(paths)))
    writers, mels, frames = {}, {}, [0] * len(paths)
    try:
        while waiting or any(o is not None for o in owner):
            for b in range(B):
                if owner[b] is None and waiting:
                    u = waiting.pop(0)
                    g = 1.0
                    if gain == 'peak' and hp.rescale:
                        if voc.input_resampler is not None:
                            raise RuntimeError('--gain peak needs recordings at the model\'s sample rate')
                        g = peak_gain(hp, chunked_peak(readers[u].chunks(chunk_samples), k), model.device)
                        readers[u].rewind()
                    voc.open(b, seed=None if seed_base is None else seed_base + u, gain=g)
                    owner[b] = u
                    writers[u] = GrowingWav(out_paths[u], hp.sample_rate)
                    mels[u] = []
            blk = np.zeros((B, chunk_samples), np.float32)
            n, fin = [0] * B, [False] * B
            for b in range(B):
                if owner[b] is None:
                    continue
                x = readers[owner[b]].read(chunk_samples)
                blk[b, :len(x)] = x
                n[b], fin[b] = len(x), readers[owner[b]].done
            res = voc.push(blk, n, fin)
            for b, chunk in res.items():
                u = owner[b]
                writers[u].append(chunk.result[-1].cpu().numpy())
                frames[u] += int(chunk.frames.shape[1])
                if mel_paths is not None:
                    mels[u].append(chunk.frames.transpose(0, 1).cpu().numpy())
                if fin[b]:
                    writers.pop(u).close()
                    if mel_paths is not None:
                        np.save(mel_paths[u], np.ascontiguousarray(np.concatenate(mels.pop(u), 0)), allow_pickle=False)
                    owner[b] = None
                    if progress is not None:
                        progress(u)
        torch.cuda.synchronize()
        voc.check()
    finally:
        for w in writers.values():
            w.close()
        voc.close()
    return frames


def main(argv=None):
    ap = argparse.ArgumentParser(description='vocode recordings chunk by chunk (analysis and synthesis push by push on the device)')
    ap.add_argument('--checkpoint', required=True, help='checkpoint directory or file of a WaveNet trained by this package')
    ap.add_argument('--input', nargs='+', required=True)
    ap.add_argument('--output_dir', required=True)
    ap.add_argument('--chunk_ms', type=float, default=100.0)
    ap.add_argument('--gain', default='1', choices=['1', 'peak'], help="1: the live case; peak: preprocessing's rescale from a first pass over the file")
    ap.add_argument('--hparams', default='')
    a = ap.parse_args(argv)
    from hparams import hparams
    from datasets.audio import get_hop_size
    from wavenet_vocoder.synthesizer import Synthesizer
    from wavenet_vocoder.train import get_checkpoint_state
    hp = hparams.parse(a.hparams)
    if hp.gin_channels > 0:
        raise RuntimeError('a globally conditioned WaveNet needs speaker ids: use LiveVocoder.open(row, g=...)')
    ckpt = get_checkpoint_state(a.checkpoint) if os.path.isdir(a.checkpoint) else a.checkpoint
    if ckpt is None:
        raise RuntimeError('no checkpoint in {}'.format(a.checkpoint))
    rate = WavReader(a.input[0]).rate
    chunk = max(1, int(round(rate * a.chunk_ms / 1000.0)))
    hop = get_hop_size(hp)
    synth = Synthesizer()
    synth.load(ckpt, hp)
    B = min(len(a.input), 32)
    model_chunk = chunk if rate == hp.sample_rate else int(chunk * hp.sample_rate / rate) + 2
    synth._ensure_capacity(B, (model_chunk // hop + 12) * hop)      # a push generates the frames of one chunk, and at the end those held back by the look-ahead
    os.makedirs(a.output_dir, exist_ok=True)
    names = [os.path.splitext(os.path.basename(p))[0] for p in a.input]
    outs = [os.path.join(a.output_dir, 'live-{}.wav'.format(nm)) for nm in names]
    frames = vocode_files(synth.model, a.input, outs, chunk, gain=a.gain, progress=lambda u: print('{} -> {}'.format(a.input[u], outs[u])))
    print('vocoded {} recordings, {} frames'.format(len(outs), sum(frames)))


if __name__ == '__main__':
    sys.exit(main())
