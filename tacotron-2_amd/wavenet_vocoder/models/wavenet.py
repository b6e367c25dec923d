"""WaveNet vocoder model -- host façade over the HIP engine.

Mirrors the public surface of the reference's ``wavenet_vocoder/models/wavenet.py:WaveNet`` (``initialize``,
``add_loss``, ``add_optimizer``, ``step``, ``incremental``, ``receptive_field``, ``variables``, the ``tower_*``
result lists) but is EAGER: where the reference builds TF graph nodes that ``session.run`` evaluates later,
these methods enqueue the HIP kernels immediately on the current stream and return device tensors.

Data-parallel training is one process per GPU (torch.distributed, backend "nccl" == RCCL): every rank owns
an identical replica, ``add_optimizer`` all-reduces the flat fp32 gradient (mean over ranks == the tower
average of wavenet.py:560-575) and every rank applies the same clip / Adam / EMA update.
"""
import numpy as np
import torch

from datasets import audio
from infolog import log
from wavenet_vocoder import _ext, util
from wavenet_vocoder.parallel import allreduce_loss_and_flags, allreduce_mean_buckets_, validation_loss
from wavenet_vocoder.util import is_mulaw, is_mulaw_quantize, is_scalar_input

from .modules import initialize_parameters, receptive_field_size


def dropout_seed(random_seed, global_step, rank=0):
    """64-bit key of a training step's dropout masks.  Every rank draws its own masks, like the reference's towers each own a
    tf.layers.dropout op (modules.py:484); rank 0 of any world size equals the single-GPU stream."""
    return (int(random_seed) * 1000003 + int(global_step) + int(rank) * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF


def stream_schedule(done, pushed, right, final):
    """Frames a stream push generates (wn_synth_stream_push): [done, pushed - right) once `right` frames of context follow them, all the
    pending frames [done, pushed) with final=True.  Returns (first, end)."""
    return done, (pushed if final else max(done, pushed - right))


def validation_summary(rows, quantized):
    """Per-utterance score rows [(sum of the negative log-likelihood, counted samples, samples with a non-zero loss)] -> the dict
    WaveNet.validate returns.  ``loss`` is the training definition over all rows together: sum / count, or sum / nonzero for the softmax
    head (``quantized``; modules.py:798).  Rows without a counted sample (an utterance of one sample) add nothing."""
    utts = [(float(s), int(round(n)), int(round(z))) for s, n, z in rows]
    live = [u for u in utts if u[1] > 0]
    tot = (float(np.sum([u[0] for u in live], dtype=np.float64)) if live else 0.0, sum(u[1] for u in live), sum(u[2] for u in live))
    return {'loss': validation_loss(tot[0], tot[1], tot[2], quantized), 'sum': tot[0], 'count': tot[1], 'nonzero': tot[2], 'utterances': utts}


def temperature_pair(hparams, temperature=None, mixture_temperature=None):
    """(tau_scale, tau_select) of the engine for this model's head.  ``temperature`` scales the logistic / normal draw of the scalar heads and
    is the class-choice temperature of the softmax head (which has no other noise); ``mixture_temperature`` is the mixture-of-logistics head's
    component-choice temperature and a ValueError with any other head.  None: the hparams value (mi355_synthesis_temperature /
    mi355_synthesis_mixture_temperature, default 1.0).  Each in [0, 2]; 0 is the deterministic decode (the engine validates the range)."""
    t = float(getattr(hparams, 'mi355_synthesis_temperature', 1.0) if temperature is None else temperature)
    mt = float(getattr(hparams, 'mi355_synthesis_mixture_temperature', 1.0) if mixture_temperature is None else mixture_temperature)
    softmax = is_mulaw_quantize(hparams.input_type)
    if softmax or int(hparams.out_channels) == 2:
        if mixture_temperature is not None or mt != 1.0:
            raise ValueError('mixture_temperature applies to the mixture-of-logistics head only (this model has the {} head)'.format(
                'softmax' if softmax else 'Gaussian'))
        return (1.0, t) if softmax else (t, 1.0)
    return (t, mt)


def fold_capacity(utt_frames, plan, hop):
    """(batch, time) an engine needs for a folded run of this plan: every row fits max_time, and the whole utterances of one length, which are
    upsampled together, fit batch x time samples (wn_synthesize_folded's WN_E_SHAPE rules)."""
    n_rows = len(plan)
    n_max = max(r[2] for r in plan) * hop
    by_len = {}
    for f in utt_frames:
        by_len[int(f)] = by_len.get(int(f), 0) + 1
    need = max(f * k * hop for f, k in by_len.items())
    return n_rows, max(n_max, -(-need // n_rows))


def unfold_features(plan, feats, hop):
    """The upsampled conditioning of every whole utterance from the rows of a folded run (Engine.upsampled_features: [n_rows, cin, n_max]): row r
    contributes the frames from its keep to the next row's keep.  Equal to the features of the one-shot run (the rows were gathered from them)."""
    out = []
    for u in sorted({r[0] for r in plan}):
        idx = [i for i, r in enumerate(plan) if r[0] == u]
        parts = []
        for k, i in enumerate(idx):
            _, first, frames, keep, _ = plan[i]
            end = plan[idx[k + 1]][3] if k + 1 < len(idx) else first + frames
            parts.append(feats[i, :, (keep - first) * hop:(end - first) * hop])
        out.append(torch.cat(parts, 1))
    return out


def _post_push(post, post_output, out, n, restart):
    """One OutputStage.push of a synthesis push: out [B, pitch] model-domain samples, n / restart per row.  Returns what post_output names: the int16
    chunk ('pcm'), the float32 one ('float') or both as (pcm, float) ('both'), [B, pitch] on the device."""
    if post_output not in ('pcm', 'float', 'both'):
        raise ValueError("post_output must be 'pcm', 'float' or 'both' (got {!r})".format(post_output))
    return post.push(out, n=n, restart=restart, pcm=post_output != 'float', float_out=post_output != 'pcm')


def _denoise_post_check(post):
    """denoise= hands the output stage decoded samples: refuse any other stage before anything is generated"""
    if post is not None and getattr(post, 'in_type', None) != 0:
        raise ValueError("denoise= decodes the samples itself: post must be an OutputStage with in_type='raw' (model.output_stage(rows, in_type='raw')), got in_type {!r}".format(
            getattr(post, 'in_type', None)))


def _denoise_push(model, ds, strength, out, n, restart, final, post, post_output):
    """One DenoiseStream.push of a synthesis push, followed by the output stage when there is one: out [B, pitch] model-domain samples, n / restart / final
    per row.  Returns (chunk, n_out): what the denoiser emitted for every row (n_out[b] samples, lagging the row's samples by less than n_fft), as the
    float32 chunk [B, pitch'] it produced (post None) or as what post_output names from post.push on it."""
    if strength is None:
        strength = float(getattr(model._hparams, 'mi355_output_denoise', 0.0))
    y, n_out = ds.push(out, n=n, restart=restart, final=final, strength=float(strength))
    if post is None:
        return y, n_out
    return _post_push(post, post_output, y, n_out, restart), n_out


def _resample_push(rs, out, n, restart, final, post, post_output, denoise, model, strength):
    """The playable chunk of a synthesis push at the output rate: the float32 chain at the model rate (denoise if given, then post's decode and de-emphasis),
    then one Resampler.push (rs: WaveNet.output_resampler; row = row of the push, restarted and ended with it), then what post_output names: the float32
    chunk, its int16 cast at rs.tail's gain, or both as (pcm, float).  Returns (chunk, n_out): n_out[b] samples of row b at the output rate."""
    if post_output not in ('pcm', 'float', 'both'):
        raise ValueError("post_output must be 'pcm', 'float' or 'both' (got {!r})".format(post_output))
    if denoise is not None:
        y, n_y = _denoise_push(model, denoise, strength, out, n, restart, final, post, 'float')
    else:
        y, n_y = _post_push(post, 'float', out, n, restart), n
    z, n_out = rs.push(y, n=n_y, restart=restart, final=final)
    if post_output == 'float':
        return z, n_out
    q = rs.tail.push(z, n=n_out, restart=restart)
    return (q if post_output == 'pcm' else (q, z)), n_out


def _resample_check(resample, post, denoise):
    """resample= works on decoded float32 samples: it needs the output stage or the denoiser in front of it"""
    if resample is not None and post is None and denoise is None:
        raise ValueError('resample= needs post= (an OutputStage: the decode and the de-emphasis at the model rate) or denoise= in front of it')


class SynthesisStream(object):
    """Generation of B utterances chunk by chunk as their mel frames arrive (WaveNet.stream): the samples are bit-identical to one
    WaveNet.incremental-style run over the concatenated frames with the same seed.  push() returns the samples whose conditioning is now
    complete, as a device tensor [B, n] (asynchronous: nothing waits for the GPU)."""

    def __init__(self, model, batch, g=None, seed=0, steps_per_graph=0, temperature=None):
        """temperature: the engine's pair (tau_scale, tau_select) for this stream's pushes (temperature_pair); None: the engine's pair as it is."""
        self.model, self.B = model, int(batch)
        self.lookahead = model.engine.stream_lookahead()
        self.done = self.pushed = 0
        self.hop = model.engine.hop
        model._ensure_packed()
        if model.global_conditioning_enabled():
            model._set_global(g, self.B)
        if temperature is not None:
            model.engine.set_temperature(*temperature)
        model.engine.stream_begin(self.B, seed=seed, steps_per_graph=steps_per_graph)
        self.closed = False

    def push(self, c_frames=None, final=False, noise=None, test_inputs=None, return_raw=False, post=None, post_output='pcm', denoise=None, denoise_strength=None, resample=None):
        """c_frames [B, cin, Tn] (None or Tn = 0: no new frames); noise [n, B, noise_per_step] / test_inputs [B, n] of the span this push
        generates (its length follows from stream_schedule and the lookahead).  post: an OutputStage (WaveNet.output_stage) of >= B rows: the
        playable chunk [B, n] -- decoded, de-emphasised, int16 at the stage's gain (post_output 'float': float32; 'both': (int16, float32)) -- is
        returned as a last element beside the samples; the stage's filter runs on from push to push, restarted at the stream's first one.
        denoise: an _ext.DenoiseStream (WaveNet.stream_denoiser) of >= B rows and max_push >= n: the samples of this push are decoded and denoised by it
        (strength denoise_strength; None: mi355_output_denoise) and what it emits goes to post, which must then be an OutputStage with in_type='raw'.  The
        playable chunk is the denoised one: it lags the samples by S - E < n_fft (DenoiseStream.ready) and the final push returns the flushed rest; without
        post it is the denoised float32 chunk.  The generated samples are the same with or without denoise.
        resample: a WaveNet.output_resampler of >= B rows, behind post and / or denoise: the playable chunk is converted to its sample rate after the
        de-emphasis and before the int16 cast (at the resampler's tail stage), lags by at most W more input samples (Resampler.ready) and the final push
        flushes; its length is what the resampler emitted.  The generated samples are the same with or without it."""
        if self.closed:
            raise RuntimeError('SynthesisStream: the stream is closed')
        if denoise is not None:
            _denoise_post_check(post)
        _resample_check(resample, post, denoise)
        m = self.model
        cc = None
        if c_frames is not None and int(c_frames.shape[-1]) > 0:
            if c_frames.dim() != 3 or c_frames.shape[0] != self.B or c_frames.shape[1] != m._hparams.cin_channels:
                raise ValueError('SynthesisStream.push: c_frames must be [B=%d, cin=%d, Tn] (got %s)' % (self.B, m._hparams.cin_channels, tuple(c_frames.shape)))
            cc = c_frames.to(m.device, torch.float32).contiguous()
        Tn = 0 if cc is None else int(cc.shape[-1])
        first, end = stream_schedule(self.done, self.pushed + Tn, self.lookahead[1], final)
        n = (end - first) * self.hop
        out = torch.empty(self.B, max(n, 1), device=m.device, dtype=torch.float32 if m.scalar_input else torch.int32)
        raw = torch.empty(self.B, m._hparams.out_channels, max(n, 1), device=m.device) if return_raw else None
        ti = None
        if test_inputs is not None:
            ti = (test_inputs.float() if m.scalar_input else test_inputs.to(torch.int32)).to(m.device).contiguous()
        got = m.engine.stream_push(cc, out, raw, None if noise is None else noise.to(m.device).contiguous(), ti, final=final)
        assert got == n
        self.pushed += Tn
        self.done = end
        if final:
            self.closed = True
        chunk = None
        if resample is not None:
            chunk, n_out = _resample_push(resample, out, [n] * self.B, None if getattr(self, '_post_started', False) else True, [final] * self.B, post, post_output,
                                          denoise, m, denoise_strength)
            self._post_started = True
            chunk = tuple(t[:, :n_out[0]] for t in chunk) if isinstance(chunk, tuple) else chunk[:, :n_out[0]]      # (every row has the same S: the same n_out)
        elif denoise is not None:
            chunk, n_out = _denoise_push(m, denoise, denoise_strength, out, [n] * self.B, None if getattr(self, '_post_started', False) else True, [final] * self.B,
                                         post, post_output)
            self._post_started = True
            chunk = tuple(t[:, :n_out[0]] for t in chunk) if isinstance(chunk, tuple) else chunk[:, :n_out[0]]      # (every row has the same S: the same n_out)
        elif post is not None:
            chunk = _post_push(post, post_output, out, [n] * self.B, None if getattr(self, '_post_started', False) else True)
            self._post_started = True
            chunk = tuple(t[:, :n] for t in chunk) if isinstance(chunk, tuple) else chunk[:, :n]
        out = out[:, :n]
        res = (out, raw[:, :, :n]) if return_raw else (out,)
        if chunk is not None:
            res = res + (chunk,)
        return res if len(res) > 1 else res[0]

    def close(self):
        """Abandon the stream (frames pushed and not yet generated are dropped)."""
        if not self.closed:
            self.model.engine.stream_end()
        self.closed = True


def slot_plan(lengths, B, tick_frames):
    """Assign utterances of `lengths` frames to the B slots of a SlotSession (no GPU): input order, lowest free slot first, a slot that finished
    at push k is refilled at push k + 1.  Every live slot receives up to `tick_frames` frames per push.  Yields, per push,
    (opens, frames, final): opens = [(slot, utterance index)] to open before the push, frames[b] / final[b] as SlotSession.push / wn_synth_slots_push
    take them (frames[b] counted from the utterance's next undelivered frame)."""
    B, tick = int(B), int(tick_frames)
    if B <= 0 or tick <= 0:
        raise ValueError('slot_plan: B and tick_frames must be positive')
    lengths = [int(n) for n in lengths]
    if any(n <= 0 for n in lengths):
        raise ValueError('slot_plan: every utterance needs at least one frame')
    nxt, owner, left = 0, [None] * B, [0] * B
    while nxt < len(lengths) or any(o is not None for o in owner):
        opens = []
        for b in range(B):
            if owner[b] is None and nxt < len(lengths):
                owner[b], left[b] = nxt, lengths[nxt]
                opens.append((b, nxt))
                nxt += 1
        frames, final = [0] * B, [False] * B
        for b in range(B):
            if owner[b] is None:
                continue
            frames[b] = min(tick, left[b])
            left[b] -= frames[b]
            if left[b] == 0:
                final[b] = True
                owner[b] = None
        yield opens, frames, final


def wide_plan(frames, rows, max_cells):
    """Cut utterances of `frames` mel frames into the runs of WaveNet.wide (no GPU): sorted by length (stable, longest first), then cut greedily into
    runs of at most `rows` utterances whose rows_in_run x longest_frames stays within `max_cells`; every run is padded to its own longest utterance
    only.  Returns (runs, perm): runs = lists of input indices, perm[i] = the position of utterance i in the concatenation of the runs.  An
    utterance longer than max_cells fits no run: ValueError naming it.  Sorting never pads more than cutting the input order into runs of `rows`:
    the k-th run's longest is the smallest possible, and a cut forced by max_cells only shortens what a run is padded to."""
    rows, max_cells = int(rows), int(max_cells)
    if rows <= 0 or max_cells <= 0:
        raise ValueError('wide_plan: rows and max_cells must be positive')
    frames = [int(f) for f in frames]
    for i, f in enumerate(frames):
        if f <= 0:
            raise ValueError('wide_plan: utterance {} has no frame'.format(i))
        if f > max_cells:
            raise ValueError('wide_plan: utterance {} ({} frames) fits no run of at most {} cells'.format(i, f, max_cells))
    order = sorted(range(len(frames)), key=lambda i: -frames[i])
    runs = []
    for i in order:
        if runs and len(runs[-1]) < rows and (len(runs[-1]) + 1) * frames[runs[-1][0]] <= max_cells:
            runs[-1].append(i)
        else:
            runs.append([i])
    perm = [0] * len(frames)
    for k, i in enumerate(order):
        perm[i] = k
    return runs, perm


def wide_padded_cells(frames, runs):
    """Cells a plan generates and throws away: every run is padded to its longest utterance."""
    return sum(len(r) * max(int(frames[i]) for i in r) - sum(int(frames[i]) for i in r) for r in runs)


class SlotSession(object):
    """B slots served by one pipeline configuration (WaveNet.slots): every slot is idle or carries ONE utterance with its own start, seed and
    global condition; utterances are opened, fed mel frames, finished and replaced independently, and a slot's samples are bit-identical to a
    one-shot run of that utterance in the same batch row.  push() returns the samples whose conditioning is now complete, per slot, as device
    tensors (asynchronous: nothing waits for the GPU).  wide: the session of WaveNet.wide_slots -- any B <= the engine's max_batch on the
    launch-per-layer path (Engine.wide_slots_begin); everything else is the same."""

    def __init__(self, model, batch, steps_per_graph=0, wide=False):
        self.model, self.B, self.wide = model, int(batch), bool(wide)
        self.lookahead = model.engine.stream_lookahead()
        self.hop = model.engine.hop
        self.done, self.pushed = [None] * self.B, [0] * self.B          # frames per live slot (None: idle)
        self._post_restart = set()                                      # slots opened since their last push: an output stage starts them from y[-1] = 0
        model._ensure_packed()
        (model.engine.wide_slots_begin if self.wide else model.engine.slots_begin)(self.B, steps_per_graph=steps_per_graph)
        self.closed = False

    def open(self, slot, g=None, seed=None, temperature=None, mixture_temperature=None):
        """Start an utterance in an idle slot (live with the next push).  g: its speaker id (int) or feature vector [gin_channels] when the model
        has global conditioning.  seed None: derived as incremental() derives it.  temperature / mixture_temperature: this utterance's sampling
        temperature (temperature_pair; None: the hparams values)."""
        m, hp = self.model, self.model._hparams
        pair = temperature_pair(hp, temperature, mixture_temperature)
        if seed is None:
            m._synth_calls = getattr(m, '_synth_calls', 0) + 1
            seed = ((int(hp.wavenet_random_seed) << 20) + m._synth_calls) * 64 + int(slot)
        gd = None
        if m.global_conditioning_enabled():
            if g is None:
                raise ValueError('SlotSession.open: the model has global conditioning: pass g')
            if hp.use_speaker_embedding:
                gd = torch.as_tensor(g, dtype=torch.int32).reshape(1).to(m.device)
            else:
                gd = torch.as_tensor(g, dtype=torch.float32).reshape(hp.gin_channels).to(m.device)
        m.engine.slot_open(slot, seed=seed, g=gd)
        m.engine.slot_temperature(slot, *pair)
        self.done[slot], self.pushed[slot] = 0, 0
        self._post_restart.add(int(slot))

    def push(self, items, return_raw=False, post=None, post_output='pcm', denoise=None, denoise_strength=None, resample=None):
        """items {slot: frames [cin, Tn]} or {slot: (frames, final)}: append the frames to the slots' utterances (final: the utterance ends, the slot
        is idle afterwards).  Returns {slot: samples [n]} (or (samples, raw [O, n]) with return_raw) for every slot named.  post: an OutputStage of
        >= B rows (row = slot): every slot's playable chunk [n] (SynthesisStream.push) follows as a last element; a slot's filter runs on from push
        to push and starts afresh at the first push after its open().  denoise: an _ext.DenoiseStream (WaveNet.stream_denoiser) of >= B rows
        (row = slot), as SynthesisStream.push: a slot's chunk is then the denoised one (its length is what the denoiser emitted, the slot's final push
        returns the flushed rest), a slot opened anew restarts its row in the denoiser together with its row in post, and an abandoned slot's row is
        restarted at the next open.  resample: a WaveNet.output_resampler of >= B rows (row = slot), as SynthesisStream.push: a slot's chunk is at its
        sample rate, a slot opened anew restarts its row there too, and the slot's final push flushes."""
        if self.closed:
            raise RuntimeError('SlotSession: the session is closed')
        if denoise is not None:
            _denoise_post_check(post)
        _resample_check(resample, post, denoise)
        m, hp = self.model, self.model._hparams
        frames, final, blocks = [0] * self.B, [False] * self.B, {}
        for b, it in items.items():
            fr, fin = it if isinstance(it, tuple) else (it, False)
            if self.done[b] is None:
                raise ValueError('SlotSession.push: slot %d is idle (open it first)' % b)
            if fr is not None and int(fr.shape[-1]) > 0:
                if fr.dim() != 2 or fr.shape[0] != hp.cin_channels:
                    raise ValueError('SlotSession.push: frames of slot %d must be [cin=%d, Tn] (got %s)' % (b, hp.cin_channels, tuple(fr.shape)))
                blocks[b] = fr
                frames[b] = int(fr.shape[-1])
            final[b] = bool(fin)
        Tn = max(frames)
        cc = None
        if Tn > 0:
            cc = torch.zeros(self.B, hp.cin_channels, Tn, device=m.device)
            for b, fr in blocks.items():
                cc[b, :, :frames[b]] = fr.to(m.device, torch.float32)
        n = [0] * self.B
        for b in items:
            first, end = stream_schedule(self.done[b], self.pushed[b] + frames[b], self.lookahead[1], final[b])
            n[b] = (end - first) * self.hop
        pitch = max(max(n), 1)
        out = torch.empty(self.B, pitch, device=m.device, dtype=torch.float32 if m.scalar_input else torch.int32)
        raw = torch.empty(self.B, hp.out_channels, pitch, device=m.device) if return_raw else None
        got = m.engine.slots_push(cc, frames, final, out, raw)
        assert got == n, (got, n)
        chunk, nc = None, n      # nc: the length of every slot's chunk
        if post is not None or denoise is not None:
            restart = [int(b in self._post_restart and b in items) for b in range(self.B)]
            if resample is not None:
                chunk, nc = _resample_push(resample, out, n, restart, [int(f) for f in final], post, post_output, denoise, m, denoise_strength)
            elif denoise is not None:
                chunk, nc = _denoise_push(m, denoise, denoise_strength, out, n, restart, [int(f) for f in final], post, post_output)
            else:
                chunk = _post_push(post, post_output, out, n, restart)
            self._post_restart -= set(items)
        res = {}
        for b in items:
            self.pushed[b] += frames[b]
            self.done[b] += n[b] // self.hop
            if final[b]:
                self.done[b] = None
            r = (out[b, :n[b]], raw[b, :, :n[b]]) if return_raw else (out[b, :n[b]],)
            if chunk is not None:
                r = r + (tuple(t[b, :nc[b]] for t in chunk) if isinstance(chunk, tuple) else chunk[b, :nc[b]],)
            res[b] = r if len(r) > 1 else r[0]
        return res

    def abandon(self, slot):
        """Drop the slot's utterance (frames pushed and not generated are lost); the slot is idle."""
        self.model.engine.slot_abandon(slot)
        self.done[slot] = None

    def check(self):
        """Wait for the last push and raise if the pipeline gave up (a half-precision pipeline whose residual stream left the half range raises
        here: switch the engine to bf16 with pipeline_dtype(False) and run the utterances again -- the re-run is the caller's)."""
        self.model.engine.synth_check()

    def close(self):
        if not self.closed:
            self.model.engine.slots_end()
        self.closed = True


def silent_conditioning_value(hp):
    """What an all-zero signal analyses to, as synthesis hands it to the model: the level floor through the analysis' own normalisation (datasets/audio.py;
    -max_abs_value under the default hparams: the pad value of wn_mel_run and of Synthesizer.synthesize), then clip_for_wavenet / normalize_for_wavenet."""
    S = audio._amp_to_db(np.zeros(1), hp) - hp.ref_level_db
    v = float(np.asarray(audio._normalize(S, hp) if hp.signal_normalization else S).reshape(-1)[0])
    lo, hi = (-hp.max_abs_value, hp.max_abs_value) if hp.symmetric_mels else (0, hp.max_abs_value)
    if hp.clip_for_wavenet:
        v = min(max(v, lo), hi)
    if hp.normalize_for_wavenet:
        v = (v - lo) / (hi - lo)
    return v


class OutputDenoiser(_ext.SpectralDenoiser):
    """WaveNet.denoiser: an _ext.SpectralDenoiser in the hparams' geometry that can fit its profile from the model's own output on silent conditioning."""

    def __init__(self, model, rows, max_samples):
        n_fft, hop = _ext.denoise_geometry(model._hparams)
        super().__init__(n_fft, hop, rows, max_samples)
        self.model = model

    def fit_from_model(self, frames=None, seed=None, speaker=None):
        """One utterance of `frames` mel frames (mi355_output_denoise_profile_frames) generated by WaveNet.incremental from conditioning held at
        silent_conditioning_value, at the temperature pair every synthesis call of this model sets on its context (the hparams'), decoded, and fitted -- all
        on the device.
        seed: of the device noise (None: derived from wavenet_random_seed); the model's synthesis-call counter is left as it was, so the utterances
        generated afterwards are those of a run without the fit.  speaker: the global condition (mi355_output_denoise_speaker)."""
        m, hp = self.model, self.model._hparams
        frames = int(frames if frames is not None else getattr(hp, 'mi355_output_denoise_profile_frames', 64))
        speaker = int(speaker if speaker is not None else getattr(hp, 'mi355_output_denoise_speaker', 0))
        T = frames * audio.get_hop_size(hp)
        if T > self.max_samples:
            raise ValueError('fit_from_model: {} frames are {} samples, the denoiser holds {}'.format(frames, T, self.max_samples))
        if m.engine is None:
            m.build(1, T, inference_only=True)
        c = torch.full((1, hp.cin_channels, frames), silent_conditioning_value(hp), dtype=torch.float32, device=m.device)
        calls = getattr(m, '_synth_calls', 0)
        noise = None
        if seed is not None:
            m._ensure_packed()
            noise = torch.empty(T, 1, m.engine.noise_per_step, device=m.device)
            m.engine.fill_noise(noise, 1, T, int(seed))
        try:
            out = m.incremental(None, c=c, g=[speaker] if m.global_conditioning_enabled() else None, time_length=T, noise=noise, check=True)
        finally:
            m._synth_calls = calls
        if is_mulaw_quantize(hp.input_type):
            out = util.inv_mulaw_quantize(out)
        elif is_mulaw(hp.input_type):
            out = util.inv_mulaw(out)
        self.fit(out.float().reshape(1, -1).contiguous(), [T])
        return self


class WaveNet(object):
    def __init__(self, hparams, init=False):
        self._hparams = hparams
        if self.local_conditioning_enabled():
            assert hparams.num_mels == hparams.cin_channels
        assert hparams.layers % hparams.stacks == 0
        if hparams.gin_channels > 0 and hparams.use_speaker_embedding:
            assert hparams.n_speakers is not None                                    # wavenet.py:154
        self.scalar_input = is_scalar_input(hparams.input_type)
        self.receptive_field = receptive_field_size(hparams.layers, hparams.stacks, hparams.kernel_size)
        self.embed_speakers = 'gc_embedding' if (hparams.gin_channels > 0 and hparams.use_speaker_embedding) else None
        self.engine = None
        self.is_training = False
        self.is_evaluating = False
        self.global_step = 0
        self._world = 1
        self._dist = None

    # ------------------------------------------------------------------ construction
    def build(self, max_batch, max_time, device=None, params=None, inference_only=False):
        """Allocate the engine (packed weights + workspace) and the flat fp32 parameter / optimiser buffers.  inference_only: a
        synthesis-only engine (no training workspace: ~1.5 KB instead of ~45 KB of HBM per (stream x sample))."""
        hp = self._hparams
        if device is None:
            device = torch.device('cuda', torch.cuda.current_device())
        self.device = device
        hop = audio.get_hop_size(hp)
        max_time = (int(max_time) + hop - 1) // hop * hop
        self.engine = _ext.Engine(hp, max_batch, max_time, inference_only=inference_only)
        self.inference_only = bool(inference_only)
        self.max_batch, self.max_time = max_batch, max_time
        if params is None:
            params = initialize_parameters(hp, self.engine.layout)
        self.params = params.to(device).contiguous()
        assert self.params.numel() == self.engine.n_params
        if inference_only:                                  # synthesis only: no gradient / Adam slots (4 x 55 MB at the paper shape)
            self.grads = self.adam_m = self.adam_v = torch.zeros(0, device=device)
        else:
            self.grads = torch.zeros_like(self.params)
            self.adam_m = torch.zeros_like(self.params)
            self.adam_v = torch.zeros_like(self.params)
        self.ema_params = self.params.clone()                # tf.train.ExponentialMovingAverage shadow (wavenet.py:473)
        self.variables = self.engine.views(self.params)      # name -> tensor view (TF layouts)
        self.gradients = None if inference_only else self.engine.views(self.grads)
        self._loss_dev = torch.zeros(1, device=device)
        self._dirty = True
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            self._dist = torch.distributed
            self._world = self._dist.get_world_size()
            self._dist.broadcast(self.params, 0)
            self.ema_params.copy_(self.params)
        log('Initializing Wavenet model.  Dimensions: ')
        log('  Receptive Field:           ({} samples / {:.1f} ms)'.format(self.receptive_field, self.receptive_field / hp.sample_rate * 1000.))
        n = sum(int(np.prod(s)) for s, _ in self.engine.layout.values())
        log('  WaveNet Parameters:        {:.3f} Million.'.format(n / 1000000))
        return self

    def _ensure_packed(self):
        if self._dirty:
            self.engine.pack_weights(self.ema_params if getattr(self, '_pack_ema', False) else self.params)
            self._dirty = False

    def use_ema_weights(self, enable=True):
        """Synthesis / evaluation with the averaged weights (what the reference intended with its shadow saver, train.py:75-83):
        from now on the engine packs ``ema_params`` instead of ``params`` (training forwards included, so only switch it on for a
        synthesis-only model or switch it off again)."""
        self._pack_ema = bool(enable)
        self._dirty = True

    # ------------------------------------------------------------------ reference-shaped API
    def initialize(self, y, c, g, input_lengths, x=None, synthesis_length=None, test_inputs=None, split_infos=None, keep_y_hat=False):
        """Train (x given), eval (y given, x None) or synthesis (neither) -- wavenet.py:218-473.  keep_y_hat (training): the forward also copies its
        y_hat [B, out_channels, T] of the whole batch to ``self._y_hat_train`` (the training summaries read it); the step itself is unchanged."""
        hp = self._hparams
        self.is_training = x is not None
        self.is_evaluating = not self.is_training and y is not None
        self.tower_y_hat, self.tower_y_target, self.tower_synth_upsampled_local_features = [], [], []
        if self.is_training:
            B, T = int(x.shape[0]), int(x.shape[-1])
            if self.engine is None:
                self.build(B, T)
            self._ensure_packed()
            rank = self._dist.get_rank() if (self._dist is not None and self._world > 1) else 0
            self._seed = dropout_seed(hp.wavenet_random_seed, self.global_step, rank)
            self.tower_y, self.tower_input_lengths, self.tower_c = [y], [input_lengths], [c]
            self._y_hat_train = torch.empty(B, hp.out_channels, T, device=self.device) if keep_y_hat else None
            self._set_global(g, B)
            self.engine.train_fwd(x.contiguous(), c.contiguous(), y.contiguous(), input_lengths, self._seed, self._loss_dev, self._y_hat_train)
            self._have_fwd = True
            return
        if self.is_evaluating:
            # item 0 of the batch, teacher forced unless wavenet_natural_eval (wavenet.py:342-405)
            idx = 0
            length = int(input_lengths[idx])
            hop = audio.get_hop_size(hp)
            length = length // hop * hop
            y0 = y[idx].reshape(-1)[:length]
            c0 = c[idx:idx + 1, :, :length // hop].contiguous()
            ti = None if hp.wavenet_natural_eval else y0.reshape(1, -1).contiguous()
            g0 = None if g is None else torch.as_tensor(g)[idx:idx + 1]
            out, raw = self.incremental(None, c=c0, g=g0, time_length=length, test_inputs=ti, return_raw=True, check=True,      # (evaluation samples at the model's own scale)
                                        temperature=1.0, mixture_temperature=None if (not self.scalar_input or hp.out_channels == 2) else 1.0)
            tgt = y0.reshape(1, -1)
            ln = torch.tensor([length], dtype=torch.int32, device=raw.device)
            self.engine.loss(raw, tgt.contiguous(), ln, 0, self._loss_dev)          # no shift: wavenet.py:497-506
            self.eval_loss = self._loss_dev.clone()
            y_hat = out.reshape(-1)
            y_target = y0
            if is_mulaw_quantize(hp.input_type):
                y_hat = util.inv_mulaw_quantize(y_hat); y_target = util.inv_mulaw_quantize(y_target)
            elif is_mulaw(hp.input_type):
                y_hat = util.inv_mulaw(y_hat); y_target = util.inv_mulaw(y_target.float())
            self.tower_y_hat.append(y_hat)
            self.tower_y_target.append(y_target)
            self.tower_eval_c = [c0[0]]
            self.tower_eval_upsampled_local_features = [self.upsampled_local_features[0]]
            return
        # synthesis: c arrives [B, Tc, num_mels] like the reference's placeholder (wavenet.py:408-465)
        assert c is not None, 'local conditioning is required'
        if c.dim() != 3:
            raise ValueError('Expected 3 dimension shape [batch_size(1), time_length, {}] for local condition features but found {}'.format(
                hp.cin_channels, tuple(c.shape)))
        cT = c.transpose(1, 2).contiguous()
        out = self.incremental(None, c=cT, g=g, time_length=None, test_inputs=test_inputs, check=True,
                               chunk_frames=int(getattr(self._hparams, 'mi355_synthesis_chunk_frames', 0)))
        if is_mulaw_quantize(hp.input_type):
            y_hat = util.inv_mulaw_quantize(out)
        elif is_mulaw(hp.input_type):
            y_hat = util.inv_mulaw(out)
        else:
            y_hat = out
        self.tower_y_hat.append(y_hat)
        self.tower_synth_upsampled_local_features.append(self.upsampled_local_features)

    def add_loss(self, flags=None):
        """wavenet.py:476-519.  The masked loss is fused into the forward call; this exposes it.  Data parallel: the reported loss is
        the mean of the per-tower losses (wavenet.py:515-516; logging and the NaN guard only -- gradients never see it), and the
        training loop's per-step flags (``flags``: a float vector, e.g. "my feeder failed") ride in the SAME small all-reduce:
        ``self.reduced_flags`` = how many ranks raised each."""
        if self.is_training:
            self.tower_loss = [self._loss_dev]
            if flags is None:
                flags = self._loss_dev.new_zeros(0)
            if self._dist is not None and self._world > 1:
                vec = allreduce_loss_and_flags(self._loss_dev, flags)
                self.loss, self.reduced_flags = vec[:1], vec[1:]
            else:
                self.loss, self.reduced_flags = self._loss_dev, flags
            return self.loss
        if self.is_evaluating:
            return self.eval_loss
        raise RuntimeError('Model not in train/eval mode but computing loss: Where did this go wrong?')

    def learning_rate_at(self, global_step):
        hp = self._hparams
        return _ext.learning_rate(hp.wavenet_lr_schedule, hp.wavenet_learning_rate, global_step,
                                  hp.wavenet_decay_rate, hp.wavenet_decay_steps, hp.wavenet_warmup)

    def add_optimizer(self, global_step=None):
        """Backward + tower-gradient mean (RCCL all-reduce) + clip + Adam + EMA -- wavenet.py:522-613."""
        if not getattr(self, '_have_fwd', False):
            raise RuntimeError('add_optimizer needs a training-mode initialize() first')
        step = self.global_step if global_step is None else int(global_step)
        self.engine.train_bwd(self.grads)
        allreduce_mean_buckets_(self.engine, self.grads)      # per bucket, as soon as it is final: overlaps the rest of the backward
        self.learning_rate = self.learning_rate_at(step)
        self.engine.optim_step(self.params, self.grads, self.adam_m, self.adam_v, self.ema_params, self.learning_rate, step)
        self._dirty = True
        self._have_fwd = False
        self.global_step = step + 1
        self.optimize = True
        return self.global_step

    def get_mask(self, input_lengths, maxlen=None):
        expand = not is_mulaw_quantize(self._hparams.input_type)
        mask = util.sequence_mask(input_lengths, max_len=maxlen, expand=expand)
        return mask[:, 1:] if not expand else mask[:, 1:, :]

    def _set_global(self, g, B):
        """Hand the global conditioning of this batch to the engine (wavenet.py:669-678): speaker ids [B] / [B,1] when the
        model owns an embedding table, else features [B, gin_channels]."""
        if not self.global_conditioning_enabled():
            return
        if g is None:
            raise ValueError('global conditioning is enabled (gin_channels > 0) but no g was given')
        g = torch.as_tensor(g, device=self.device)
        if self.embed_speakers is not None:
            g = g.reshape(B).to(torch.int32)
        else:
            g = g.reshape(B, self._hparams.gin_channels).to(torch.float32)
        self.engine.set_global_condition(g.contiguous())

    @property
    def embedding_table(self):
        return self.variables['gc_embedding'] if self.embed_speakers is not None else None

    def has_speaker_embedding(self):
        return self.embed_speakers is not None

    def local_conditioning_enabled(self):
        return self._hparams.cin_channels > 0

    def global_conditioning_enabled(self):
        return self._hparams.gin_channels > 0

    def step(self, x, c=None, g=None, softmax=False):
        """Teacher-forced parallel forward: x [B,Cin,T] (or ids [B,T]), c [B,cin,Tc] -> [B,O,T] (wavenet.py:650-721)."""
        B, T = int(x.shape[0]), int(x.shape[-1])
        if self.engine is None:
            self.build(B, T)
        self._ensure_packed()
        y_hat = torch.empty(B, self._hparams.out_channels, T, device=x.device)
        lengths = torch.full((B,), T, dtype=torch.int32, device=x.device)
        dummy_y = x.reshape(B, T).contiguous() if not self.scalar_input else x.reshape(B, T, 1).contiguous()
        self._set_global(g, B)
        self.engine.train_fwd(x.contiguous(), c.contiguous(), dummy_y, lengths, 0, None, y_hat)
        self._have_fwd = False
        return torch.softmax(y_hat, dim=1) if softmax else y_hat

    def validate(self, batches):
        """Held-out likelihood: one batched dropout-free teacher-forced forward (engine.eval_fwd) per feeder-format batch (x, y, lengths, c, g)
        of ``batches`` -- Feeder.validation_batches() -- with the parameters as currently packed (no re-pack: the weights eval_step uses).
        Returns {'loss', 'sum', 'count', 'nonzero', 'utterances': [(sum, count, nonzero), ...]} (validation_summary), the rows in the order the
        utterances arrived.  Nothing waits for the GPU until the one device-to-host copy of all rows at the end.  A pending backward is
        dropped: call it between training steps."""
        if self.engine is None:
            raise RuntimeError('WaveNet.validate: call build() / initialize() first')
        if getattr(self, 'inference_only', False):
            raise RuntimeError('WaveNet.validate needs a training engine (build(inference_only=False))')
        self._ensure_packed()
        rows = []
        for x, y, lengths, c, g in batches:
            B = int(lengths.shape[0])
            self._set_global(g, B)
            st = torch.empty(B, 3, device=self.device)
            self.engine.eval_fwd(x.contiguous(), c.contiguous(), y.contiguous(), lengths.contiguous(), st)
            rows.append(st)
        self._have_fwd = False
        host = torch.cat(rows).cpu().tolist() if rows else []
        return validation_summary(host, is_mulaw_quantize(self._hparams.input_type))

    def incremental(self, initial_input, c=None, g=None, time_length=100, test_inputs=None, softmax=True, quantize=True,
                    log_scale_min=-7.0, log_scale_min_gauss=-7.0, noise=None, return_raw=False, check=False, chunk_frames=0,
                    temperature=None, mixture_temperature=None, post=None):
        """Fast-WaveNet generation with ring-buffer queues: c [B,cin,Tc] -> samples [B,T] (wavenet.py:724-911).
        ``initial_input`` is accepted for signature parity; generation always starts from the reference's silence
        frame (wavenet.py:433-445).  ``noise`` [T,B,noise_per_step] may be supplied for reproducible draws.
        ``check``: wait for the generation and verify it; if the persistent pipeline gave up on a hand-off (a workgroup was not
        resident -- the reference's loop cannot fail this way) the batch is re-run ONCE on the launch-per-layer graph path.
        ``chunk_frames`` > 0: every group goes through a stream (wn_synth_stream_push) fed this many mel frames at a time -- the same samples,
        bit for bit (same seed and stream grouping), as the one call per group of chunk_frames = 0.
        ``temperature`` / ``mixture_temperature``: sampling temperature (temperature_pair; None: the hparams values), for device noise and for
        ``noise`` alike; the fallback re-runs keep it.
        ``post``: an OutputStage of >= B rows: the whole utterances through its finish() -- (float32 [B, T] de-emphasised, int16 [B, T] peak-normalised
        as save_wavenet_wav does), returned as a last element beside the samples."""
        hp = self._hparams
        pair = temperature_pair(hp, temperature, mixture_temperature)
        B, Tc = int(c.shape[0]), int(c.shape[-1])
        hop = audio.get_hop_size(hp)
        T = Tc * hop
        if self.engine is None:
            self.build(B, T)
        self._ensure_packed()
        self.engine.set_temperature(*pair)                 # host state of the engine: every run below, the re-runs included, reads it
        dev = c.device
        # noise None: drawn on the device (Philox keyed by (wavenet_random_seed, call counter)): U(1e-5, 1 - 1e-5) as mixture.py:91,104,
        # standard normal for the Gaussian head (gaussian.py:50), Gumbel uniforms for tf.multinomial (wavenet.py:865)
        self._synth_calls = getattr(self, '_synth_calls', 0) + 1
        seed = (int(hp.wavenet_random_seed) << 20) + self._synth_calls
        out = torch.empty(B, T, device=dev, dtype=torch.float32 if self.scalar_input else torch.int32)
        raw = torch.empty(B, hp.out_channels, T, device=dev) if return_raw else None
        ti = None
        if test_inputs is not None:
            ti = test_inputs.reshape(B, -1)[:, :T]
            ti = (ti.float() if self.scalar_input else ti.to(torch.int32)).contiguous()
            assert ti.shape[1] == T, 'teacher-forcing inputs must cover the whole synthesis length'
        spg = int(getattr(hp, 'mi355_steps_per_graph', 0))
        cc = c.contiguous().float()
        feats = torch.empty(B, hp.cin_channels, T, device=dev)
        gt = None
        if self.global_conditioning_enabled():
            if g is None:
                raise ValueError('global conditioning is enabled (gin_channels > 0) but no g was given')
            gt = torch.as_tensor(g, device=self.device).reshape(B, -1)

        def run_stream(b0, b1, nz, spg_, sd):
            # one group through a stream: chunk_frames mel frames per push (the samples of a push land in contiguous scratch, then in place)
            nb = b1 - b0
            right = self.engine.stream_lookahead()[1]
            self.engine.stream_begin(nb, seed=sd, steps_per_graph=spg_)
            done = pushed = 0
            for f0 in range(0, Tc, int(chunk_frames)):
                f1 = min(Tc, f0 + int(chunk_frames))
                final = f1 == Tc
                first, end = stream_schedule(done, f1, right, final)
                t0, n = first * hop, (end - first) * hop
                o = torch.empty(nb, max(n, 1), device=dev, dtype=out.dtype)
                r = None if raw is None else torch.empty(nb, hp.out_channels, max(n, 1), device=dev)
                got = self.engine.stream_push(cc[b0:b1, :, f0:f1].contiguous(), o, r, None if nz is None else nz[t0:t0 + n].contiguous(),
                                              None if ti is None else ti[b0:b1, t0:t0 + n].contiguous(), final=final)
                assert got == n
                if n > 0:
                    out[b0:b1, t0:t0 + n] = o[:, :n]
                    if raw is not None:
                        raw[b0:b1, :, t0:t0 + n] = r[:, :, :n]
                    fe = torch.empty(nb, hp.cin_channels, n, device=dev)
                    self.engine.upsampled_features(fe)
                    feats[b0:b1, :, t0:t0 + n] = fe
                done, pushed = end, f1

        def run(spg_):
            # The persistent pipeline pipelines the streams of a run through its layer ring: 10 streams at the wall time of one (34 - 37 us
            # per sample: real time at 22.05 kHz), every further stream + 3.6 us per sample (profiles/r5u_pipe_batch_scaling.txt) -- one run
            # of 20 streams (hparams.py: wavenet_synthesis_batch_size = 20) takes 2.0x the wall time of 8 where three groups of 8 took 3x.
            # So: the whole batch in ONE run when its per-stream LDS state fits (wn_synth_pipe_eligible), else groups of 8 (streams are
            # independent: wavenet.py:237-239 splits them over towers).  Models the pipeline does not fit take the launch-per-layer graph
            # path, whose time per step is nearly independent of the batch: up to 32 streams per run.
            group = min(B, 32)
            piped = False
            if spg_ <= 0:                   # the largest run of <= B streams the pipeline takes (an inference-only context is pre-sized: it never grows)
                g = group
                while g > 0 and not self.engine.pipeline_eligible(g):
                    g -= 1
                if g > 0:
                    piped, group = True, g
            for b0 in range(0, B, group):
                b1 = min(B, b0 + group)
                nz = None if noise is None else noise[:, b0:b1].contiguous()
                if gt is not None:
                    self._set_global(gt[b0:b1], b1 - b0)                                # wavenet.py:766-777
                if chunk_frames > 0:
                    run_stream(b0, b1, nz, spg_, seed * 64 + b0 // group)
                    continue
                self.engine.synthesize(cc[b0:b1].contiguous(), nz, out[b0:b1], None if raw is None else raw[b0:b1], None if ti is None else ti[b0:b1].contiguous(),
                                       steps_per_graph=spg_, seed=seed * 64 + b0 // group)
                self.engine.upsampled_features(feats[b0:b1])
            return group

        def attempt(spg_):
            grp = run(spg_)
            if check:
                torch.cuda.synchronize()
                self.engine.synth_check()
            return grp

        try:
            group = attempt(spg)
        except _ext.WnError as e:
            out_of_range = 'half-precision range' in str(e)
            if not check or self.engine.synth_path != 'pipeline' or not ('timed out' in str(e) or out_of_range):
                raise
            self.synth_fallbacks = getattr(self, 'synth_fallbacks', 0) + 1
            torch.cuda.synchronize()
            try:
                self.engine.synth_check()          # (a flag of a later group of the same batch may still be pending)
            except _ext.WnError:
                pass
            if out_of_range:                       # the residual stream of this model exceeds 65504 somewhere: bf16 storage (8 exponent bits) from now on
                log('WaveNet synthesis: {} -- re-running this batch with bf16 pipeline storage'.format(e))
                self.engine.pipeline_dtype(False)
                group = attempt(spg)
            else:
                log('WaveNet synthesis: {} -- re-running this batch on the launch-per-layer graph path'.format(e))
                group = attempt(32)
        if getattr(self, '_logged_synth_path', None) != (self.engine.synth_path, pair):
            self._logged_synth_path = (self.engine.synth_path, pair)
            log('WaveNet synthesis path: {} ({} streams per run{})'.format(
                self.engine.synth_path, group, '' if pair == (1.0, 1.0) else '; sampling temperature {:g}, choice temperature {:g}'.format(*pair)))
        self.upsampled_local_features = feats
        res = (out, raw) if return_raw else (out,)
        if post is not None:
            res = res + (post.finish(out, [T] * B),)
        return res if len(res) > 1 else res[0]

    def folded(self, c_list, g=None, rows=20, warm=4, fade=2, min_keep=40, fade_kind='equal_power', temperature=None, mixture_temperature=None, noise=None,
               test_inputs=None, return_rows=False, check=False, post=None):
        """Folded ("batched") generation: every utterance of c_list ([cin, F_u] mel frames each) is cut into overlapping rows, the rows run side by side as
        ONE batch -- each from a cold start, `warm` frames before the part it contributes -- and are cross-faded (`fade` frames; 'equal_power' or 'linear')
        back into one waveform per utterance on the device (wn_synthesize_folded).  rows: the number of rows of the run (<= 32; the planner, _ext.fold_plan,
        gives every utterance one and the rest to the longest, never fewer than min_keep new frames per row), or an explicit plan [(utt, first, frames,
        keep, fade)].  Returns a list of float waveforms in [-1, 1] (decoded: not the model domain); return_rows: also a dict with the plan, the rows'
        model-domain samples, raw outputs and upsampled features.  g: one speaker id / feature row per utterance.  noise [n_max, n_rows, noise_per_step] /
        test_inputs (one model-domain tensor [F_u * hop] per utterance) as incremental(); the seed is derived as incremental() derives it (row r draws the
        one-stream noise of seed + r).  check: wait and verify; a pipeline run that gave up on a hand-off is re-run ONCE on the launch-per-layer path.
        rows = 20 is the measured minimum of the wall time of a 5 s utterance on the paper model (profiles/fold_timing.json; 12 rows are within its spread).
        An utterance in one row is its one-shot run.  The defaults (~0.5 s per row, 50 ms warm-up, 25 ms fade at hop 275) follow WaveRNN practice; nobody
        has listened to them on a trained model of this tree.
        post: an OutputStage with in_type 0 ('raw': the waveforms are decoded already) of >= len(c_list) rows: the waveforms through its finish(); a list of
        (float32 de-emphasised, int16 peak-normalised) per utterance follows as a last element."""
        hp = self._hparams
        pair = temperature_pair(hp, temperature, mixture_temperature)
        hop = audio.get_hop_size(hp)
        U = len(c_list)
        if U < 1:
            raise ValueError('WaveNet.folded: no utterance')
        frames = [int(c.shape[-1]) for c in c_list]
        for c in c_list:
            if c.dim() != 2 or int(c.shape[0]) != hp.cin_channels or int(c.shape[1]) < 1:
                raise ValueError('WaveNet.folded: every utterance must be [cin={}, frames >= 1] (got {})'.format(hp.cin_channels, tuple(c.shape)))
        if post is not None and post.in_type != 0:
            raise ValueError("WaveNet.folded: post must be an output stage of in_type 'raw' (the folded waveform is decoded already)")
        if fade_kind not in _ext.FADE_KINDS:
            raise ValueError("WaveNet.folded: fade_kind must be 'equal_power' or 'linear' (got {!r})".format(fade_kind))
        try:
            if isinstance(rows, int):
                if not U <= rows <= 32:
                    raise ValueError('WaveNet.folded: rows = {} outside [{} utterances, 32]'.format(rows, U))
                plan = _ext.fold_plan(frames, rows, warm, fade, min_keep)
            else:
                plan = [tuple(int(v) for v in r) for r in rows]
                if len(plan) > 32:
                    raise ValueError('WaveNet.folded: {} rows (at most 32)'.format(len(plan)))
                _ext.fold_check(frames, plan)
        except _ext.WnError as e:
            raise ValueError(str(e))
        n_rows, n_max, F_max = len(plan), max(r[2] for r in plan) * hop, max(frames)
        if g is None and self.global_conditioning_enabled():
            raise ValueError('global conditioning is enabled (gin_channels > 0) but no g was given')
        if test_inputs is not None and len(test_inputs) != U:
            raise ValueError('WaveNet.folded: test_inputs needs one tensor per utterance')
        if self.engine is None:
            self.build(*fold_capacity(frames, plan, hop), inference_only=True)
        self._ensure_packed()
        self.engine.set_temperature(*pair)
        dev = self.device
        self._synth_calls = getattr(self, '_synth_calls', 0) + 1
        seed = ((int(hp.wavenet_random_seed) << 20) + self._synth_calls) * 64
        cc = torch.zeros(U, hp.cin_channels, F_max, device=dev)
        for u, c in enumerate(c_list):
            cc[u, :, :frames[u]] = c.to(dev, torch.float32)
        T_max = F_max * hop
        wav = torch.zeros(U, T_max, device=dev)
        dt = torch.float32 if self.scalar_input else torch.int32
        ti = None
        if test_inputs is not None:
            ti = torch.zeros(U, T_max, device=dev, dtype=dt)
            for u, t in enumerate(test_inputs):
                t = t.reshape(-1)[:frames[u] * hop]
                assert t.shape[0] == frames[u] * hop, 'teacher-forcing inputs must cover the whole synthesis length'
                ti[u, :t.shape[0]] = t.to(dev, dt)
        gt = None
        if self.global_conditioning_enabled():
            gt = torch.as_tensor(g, device=dev)
            gt = (gt.reshape(U).to(torch.int32) if self.embed_speakers is not None else gt.reshape(U, hp.gin_channels).to(torch.float32)).contiguous()
        out_rows = torch.zeros(n_rows, n_max, device=dev, dtype=dt) if return_rows else None
        out_raw = torch.zeros(n_rows, hp.out_channels, n_max, device=dev) if return_rows else None
        nz = None if noise is None else noise.to(dev, torch.float32).contiguous()
        spg = int(getattr(hp, 'mi355_steps_per_graph', 0))

        def attempt(spg_):
            self.engine.synthesize_folded(cc, frames, plan, wav, fade_kind=fade_kind, g=gt, noise=nz, seed=seed, test_inputs=ti, out_rows=out_rows, out_raw=out_raw,
                                          steps_per_graph=spg_)
            if check:
                torch.cuda.synchronize()
                self.engine.synth_check()

        try:
            attempt(spg)
        except _ext.WnError as e:
            out_of_range = 'half-precision range' in str(e)
            if not check or self.engine.synth_path != 'pipeline' or not ('timed out' in str(e) or out_of_range):
                raise
            self.synth_fallbacks = getattr(self, 'synth_fallbacks', 0) + 1
            torch.cuda.synchronize()
            if out_of_range:
                log('WaveNet folded synthesis: {} -- re-running with bf16 pipeline storage'.format(e))
                self.engine.pipeline_dtype(False)
                attempt(spg)
            else:
                log('WaveNet folded synthesis: {} -- re-running on the launch-per-layer graph path'.format(e))
                attempt(32)
        if getattr(self, '_logged_fold', None) != (self.engine.synth_path, n_rows):
            self._logged_fold = (self.engine.synth_path, n_rows)
            log('WaveNet folded synthesis: {} utterance(s) in {} rows of <= {} samples, path {}'.format(U, n_rows, n_max, self.engine.synth_path))
        wavs = [wav[u, :frames[u] * hop] for u in range(U)]
        posts = None
        if post is not None:
            py, pq = post.finish(wav, [f * hop for f in frames])
            posts = [(py[u, :frames[u] * hop], pq[u, :frames[u] * hop]) for u in range(U)]
        if not return_rows:
            return wavs if post is None else (wavs, posts)
        feats = torch.empty(n_rows, hp.cin_channels, n_max, device=dev)
        self.engine.upsampled_features(feats)
        info = {'plan': plan, 'rows': out_rows, 'raw': out_raw, 'features': feats, 'seed': seed}
        return (wavs, info) if post is None else (wavs, info, posts)

    def wide(self, c_list, g=None, rows=64, temperature=None, mixture_temperature=None, noise=None, test_inputs=None, return_raw=False, post=None, check=True):
        """Wide generation for offline work: the utterances of c_list ([cin, F_u] mel frames each, any lengths: the layout folded([c]) takes) in launch-per-layer
        runs of up to `rows` utterances -- `rows` may exceed 32 (Engine.synthesize_wide) -- planned by wide_plan: longest first, every run padded to its own
        longest utterance.  A stream's samples are those of incremental() on the launch-per-layer path with the same noise; they do not depend on the run's
        width.  Returns (samples, info): one model-domain tensor [F_u * hop] per utterance in input order (floats, or class ids of the softmax head), and
        info = {'plan': (runs, perm), 'seeds': one per run, 'features': the upsampled conditioning [cin, F_u * hop] per utterance} plus 'raw' ([O, F_u * hop]
        per utterance; return_raw) and 'post' ((float32 de-emphasised, int16 peak-normalised) per utterance through post.finish(); post: an OutputStage
        of this model's input type with >= rows rows).  g: one speaker id / feature row per utterance.  noise: None (drawn on the device; the seed of run r
        derives from (wavenet_random_seed, the synthesis-call counter, r), so two fresh models agree) or one tensor [T_run, n_run, noise_per_step] per run
        of the plan; test_inputs: one model-domain tensor [F_u * hop] per utterance.  check: wait for every run and verify it.
        Without an engine, an inference-only one is built for the largest run.  Memory: see wn_synthesize_wide (the queues take 16.8 MB per stream on the
        paper model, the conditioning ~0.5 KB per stream-sample)."""
        hp = self._hparams
        pair = temperature_pair(hp, temperature, mixture_temperature)
        hop = audio.get_hop_size(hp)
        U = len(c_list)
        if U < 1:
            raise ValueError('WaveNet.wide: no utterance')
        for c in c_list:
            if c.dim() != 2 or int(c.shape[0]) != hp.cin_channels or int(c.shape[1]) < 1:
                raise ValueError('WaveNet.wide: every utterance must be [cin={}, frames >= 1] (got {})'.format(hp.cin_channels, tuple(c.shape)))
        frames = [int(c.shape[-1]) for c in c_list]
        if g is None and self.global_conditioning_enabled():
            raise ValueError('global conditioning is enabled (gin_channels > 0) but no g was given')
        if test_inputs is not None and len(test_inputs) != U:
            raise ValueError('WaveNet.wide: test_inputs needs one tensor per utterance')
        rows = int(rows)
        if self.engine is None:
            runs, perm = wide_plan(frames, rows, rows * max(frames))
            self.build(max(len(r) for r in runs), max(frames) * hop, inference_only=True)
        else:
            runs, perm = wide_plan(frames, min(rows, self.max_batch), self.max_batch * (self.max_time // hop))
        if noise is not None and len(noise) != len(runs):
            raise ValueError('WaveNet.wide: noise needs one tensor per run of the plan ({} runs)'.format(len(runs)))
        self._ensure_packed()
        self.engine.set_temperature(*pair)
        dev = self.device
        self._synth_calls = getattr(self, '_synth_calls', 0) + 1
        base = ((int(hp.wavenet_random_seed) << 20) + self._synth_calls) << 16
        dt = torch.float32 if self.scalar_input else torch.int32
        spg = int(getattr(hp, 'mi355_steps_per_graph', 0))
        gt = None
        if self.global_conditioning_enabled():
            gt = torch.as_tensor(g, device=dev)
            gt = gt.reshape(U).to(torch.int32) if self.embed_speakers is not None else gt.reshape(U, hp.gin_channels).to(torch.float32)
        samples, feats, raws, posts, seeds = [None] * U, [None] * U, [None] * U, [None] * U, []
        for r, run in enumerate(runs):
            n, F = len(run), frames[run[0]]
            T = F * hop
            cc = torch.zeros(n, hp.cin_channels, F, device=dev)
            for k, u in enumerate(run):
                cc[k, :, :frames[u]] = c_list[u].to(dev, torch.float32)
            ti = None
            if test_inputs is not None:
                ti = torch.zeros(n, T, device=dev, dtype=dt)
                for k, u in enumerate(run):
                    t = test_inputs[u].reshape(-1)[:frames[u] * hop]
                    assert t.shape[0] == frames[u] * hop, 'teacher-forcing inputs must cover the whole synthesis length'
                    ti[k, :t.shape[0]] = t.to(dev, dt)
            if gt is not None:
                self._set_global(gt[torch.as_tensor(run, device=dev)], n)
            out = torch.empty(n, T, device=dev, dtype=dt)
            raw = torch.empty(n, hp.out_channels, T, device=dev) if return_raw else None
            seeds.append(base + r)
            self.engine.synthesize_wide(cc, None if noise is None else noise[r].to(dev, torch.float32).contiguous(), out, raw, ti, steps_per_graph=spg, seed=seeds[-1])
            fe = torch.empty(n, hp.cin_channels, T, device=dev)
            self.engine.upsampled_features(fe)
            if check:
                torch.cuda.synchronize()
                self.engine.synth_check()
            pp = post.finish(out, [frames[u] * hop for u in run]) if post is not None else None
            for k, u in enumerate(run):
                m = frames[u] * hop
                samples[u], feats[u] = out[k, :m], fe[k, :, :m]
                if raw is not None:
                    raws[u] = raw[k, :, :m]
                if pp is not None:
                    posts[u] = (pp[0][k, :m], pp[1][k, :m])
        if getattr(self, '_logged_wide', None) != (len(runs), max(len(r) for r in runs)):
            self._logged_wide = (len(runs), max(len(r) for r in runs))
            log('WaveNet wide synthesis: {} utterance(s) in {} run(s) of <= {} streams, path {}'.format(U, len(runs), self._logged_wide[1], self.engine.synth_path))
        info = {'plan': (runs, perm), 'seeds': seeds, 'features': feats}
        if return_raw:
            info['raw'] = raws
        if post is not None:
            info['post'] = posts
        return samples, info

    def output_stage(self, rows, **kw):
        """An _ext.OutputStage of `rows` rows for this model's samples (in_type and de-emphasis from the hparams; gain: mi355_output_gain): the post=
        argument of incremental / folded (in_type='raw') / SynthesisStream.push / SlotSession.push."""
        kw.setdefault('gain', float(getattr(self._hparams, 'mi355_output_gain', 1.0)))
        return _ext.OutputStage(self._hparams, rows, **kw)

    def reconstruction_check(self, rows, max_samples, preemphasis=None, alarm_db=None):
        """A ReconstructionCheck (wavenet_vocoder/reconstruction.py) for up to `rows` utterances of up to `max_samples` samples of this model: the
        mel of generated audio against the conditioning it was generated from, per frame and per utterance, on the device.  preemphasis None:
        hparams.preemphasis if hparams.preemphasize else 0, as preprocessing analyses; alarm_db None: mi355_reconstruction_alarm_db.  ValueError when
        cin_channels != num_mels (the conditioning is no mel of this analysis)."""
        from wavenet_vocoder.reconstruction import ReconstructionCheck
        return ReconstructionCheck(self._hparams, rows, max_samples, preemphasis=preemphasis, alarm_db=alarm_db)

    def alignment_check(self, rows, max_samples, band=None):
        """An AlignmentCheck (wavenet_vocoder/alignment.py) for up to `rows` pairs of signals of up to `max_samples` samples each: a generated utterance
        against a recording of another length and timing, aligned by dynamic time warping over the mel cepstra and scored along the path, on the device;
        band None: mi355_alignment_band."""
        from wavenet_vocoder.alignment import AlignmentCheck
        return AlignmentCheck(self._hparams, rows, max_samples, band=band)

    def pitch_check(self, rows, max_samples):
        """A PitchCheck (wavenet_vocoder/pitch.py) for up to `rows` utterances of up to `max_samples` samples: F0 and voicing of generated audio against
        a recording in the same domain, per utterance, on the device; the geometry comes from the hparams (mi355_pitch_*)."""
        from wavenet_vocoder.pitch import PitchCheck
        return PitchCheck(self._hparams, rows, max_samples)

    def griffin_lim(self, rows, max_frames):
        """An _ext.GriffinLim for up to `rows` mels of up to `max_frames` frames (csrc/wn_griffin.hip): the model-free inversion of this model's
        conditioning, the baseline its output is compared with; geometry, levels, power and the pseudo-inverse of the mel filters from the hparams."""
        return _ext.GriffinLim(self._hparams, rows, max_frames)

    def denoiser(self, rows, max_samples):
        """An OutputDenoiser for up to `rows` decoded utterances of up to `max_samples` samples of this model (csrc/wn_denoise.hip): the bias denoiser of
        sampled vocoders; geometry from the hparams (mi355_output_denoise_fft / _hop).  .fit(wav, lengths) / .fit_from_model(frames, seed, speaker) set the
        noise profile, .profile reads or sets it as numpy, .apply(wav, lengths, strength, out=None) subtracts it."""
        return OutputDenoiser(self, rows, max_samples)

    def stream_denoiser(self, rows, max_push, source=None):
        """An _ext.DenoiseStream of `rows` rows for pushes of up to `max_push` samples per row (csrc/wn_denoise_stream.hip): the denoise= argument of
        SynthesisStream.push / SlotSession.push.  Geometry from the hparams (mi355_output_denoise_fft / _hop), in_type from hparams.input_type (it decodes
        the model's samples itself).  source: a fitted OutputDenoiser (WaveNet.denoiser) whose profile it takes, device to device; None: set one with
        .set_profile(numpy) or .take_profile(denoiser) before the first push."""
        n_fft, hop = _ext.denoise_geometry(self._hparams)
        ds = _ext.DenoiseStream(n_fft, hop, rows, max_push, self._hparams.input_type)
        if source is not None:
            ds.take_profile(source)
        return ds

    def output_resampler(self, rows, max_push, sample_rate):
        """An _ext.Resampler of `rows` rows from hparams.sample_rate to `sample_rate` for pushes (or whole rows) of up to `max_push` samples per row
        (csrc/wn_resample.hip): the resample= argument of SynthesisStream.push / SlotSession.push, and what Synthesizer runs when
        mi355_output_sample_rate is set.  Its .tail is a raw OutputStage without de-emphasis at mi355_output_gain: the int16 cast behind the conversion.
        max_push counts what reaches the resampler in one call: with denoise= in front, a final push can flush up to n_fft samples more."""
        rs = _ext.Resampler(int(self._hparams.sample_rate), int(sample_rate), rows, max_push)
        rs.tail = self.output_stage(rows, in_type='raw', deemphasis=0.0)
        return rs

    def mel_stream(self, rows, max_push, preemphasis=None):
        """An _ext.MelStream of `rows` rows for pushes of up to `max_push` samples per row (csrc/wn_mel_stream.hip): the analysis of preprocessing on
        recordings that arrive chunk by chunk, the front end of wavenet_vocoder.live.LiveVocoder.  preemphasis None: hparams.preemphasis if
        hparams.preemphasize else 0, as preprocessing analyses."""
        hp = self._hparams
        if preemphasis is None:
            preemphasis = float(hp.preemphasis) if hp.preemphasize else 0.0
        return _ext.MelStream(hp, rows, max_push, preemphasis=preemphasis)

    def train_stats(self):
        """The model's _ext.TrainStats (csrc/wn_stats.hip), built at the first call: histograms of up to max_batch rows of max_time samples and the
        per-tensor statistics of a flat buffer in the engine's layout (``grads``, ``params``, the Adam slots)."""
        if self.engine is None:
            raise RuntimeError('WaveNet.train_stats: call build() / initialize() first')
        if getattr(self, '_train_stats', None) is None:
            self._train_stats = _ext.TrainStats(self.max_batch, self.max_time, self.engine.layout)
        return self._train_stats

    def train_outputs(self, y, step):
        """The kept training forward (initialize(keep_y_hat=True)) decoded as the reference's training tower decodes it for its summaries
        (wavenet.py:296-328): arg-max + inv_mulaw_quantize for the softmax head, one draw of the scalar heads' distribution (inv_mulaw where the input
        type asks for it), next to the targets decoded the same way.  The draw's noise comes from a generator of its own seeded from
        (wavenet_random_seed, step): the global generator, and with it the run, are untouched.  Returns (outputs, targets), float32 [B, T] each."""
        hp = self._hparams
        y_hat = getattr(self, '_y_hat_train', None)
        if y_hat is None:
            raise RuntimeError('WaveNet.train_outputs: the last training initialize() did not keep its y_hat (keep_y_hat=True)')
        B, T = int(y_hat.shape[0]), int(y_hat.shape[-1])
        if is_mulaw_quantize(hp.input_type):
            return util.inv_mulaw_quantize(_ext.argmax_channels(y_hat)), util.inv_mulaw_quantize(y.reshape(B, T))
        gen = torch.Generator(device=y_hat.device)
        gen.manual_seed((int(hp.wavenet_random_seed) * 1000003 + int(step)) & 0x7FFFFFFFFFFFFFFF)
        nps = self.engine.noise_per_step
        if hp.out_channels == 2:
            noise = torch.randn(T, B, nps, device=y_hat.device, generator=gen)
        else:
            noise = torch.rand(T, B, nps, device=y_hat.device, generator=gen) * (1 - 2e-5) + 1e-5
        out = torch.empty(B, T, device=y_hat.device)
        self.engine.sample(y_hat, noise, out)
        target = y.reshape(B, T).float().contiguous()
        if is_mulaw(hp.input_type):
            out, target = util.inv_mulaw(out), util.inv_mulaw(target)
        return out, target

    def slots(self, batch, steps_per_graph=None):
        """Open a SlotSession of `batch` slots (<= 32, the model's engine must have been built for them): independent utterances that join and
        leave one running batch."""
        hp = self._hparams
        if self.engine is None:
            raise RuntimeError('WaveNet.slots: call build() / initialize() first')
        spg = int(getattr(hp, 'mi355_steps_per_graph', 0)) if steps_per_graph is None else int(steps_per_graph)
        return SlotSession(self, batch, steps_per_graph=spg)

    def wide_slots(self, batch, steps_per_graph=None):
        """Open a SlotSession of any `batch` <= the engine's max_batch slots on the launch-per-layer path (Engine.wide_slots_begin): continuous
        batching at the width of WaveNet.wide.  The conditioning is upsampled push by push, so the engine's max_time need only cover one push."""
        hp = self._hparams
        if self.engine is None:
            raise RuntimeError('WaveNet.wide_slots: call build() / initialize() first')
        spg = int(getattr(hp, 'mi355_steps_per_graph', 0)) if steps_per_graph is None else int(steps_per_graph)
        return SlotSession(self, batch, steps_per_graph=spg, wide=True)

    def stream(self, batch, g=None, seed=None, steps_per_graph=None, temperature=None, mixture_temperature=None):
        """Open a SynthesisStream of `batch` utterances (<= 32, the model's engine must have been built for them).  seed None: derived as
        incremental() derives it.  temperature / mixture_temperature: as incremental()."""
        hp = self._hparams
        pair = temperature_pair(hp, temperature, mixture_temperature)
        if self.engine is None:
            self.build(batch, audio.get_hop_size(hp) * 64, inference_only=True)
        if seed is None:
            self._synth_calls = getattr(self, '_synth_calls', 0) + 1
            seed = ((int(hp.wavenet_random_seed) << 20) + self._synth_calls) * 64
        spg = int(getattr(hp, 'mi355_steps_per_graph', 0)) if steps_per_graph is None else int(steps_per_graph)
        return SynthesisStream(self, batch, g=g, seed=seed, steps_per_graph=spg, temperature=pair)

    # ------------------------------------------------------------------ checkpoint state
    def state_dict(self):
        return {'params': self.params.detach().cpu(), 'ema': self.ema_params.detach().cpu(), 'adam_m': self.adam_m.detach().cpu(),
                'adam_v': self.adam_v.detach().cpu(), 'global_step': self.global_step,
                'layout': {k: (tuple(s), int(o)) for k, (s, o) in self.engine.layout.items()}}

    def load_state_dict(self, sd):
        for name, dst in (('params', self.params), ('ema', self.ema_params), ('adam_m', self.adam_m), ('adam_v', self.adam_v)):
            if getattr(self, 'inference_only', False) and name.startswith('adam'):
                continue
            src = sd[name]
            if src.numel() != dst.numel():
                raise ValueError('checkpoint tensor %s has %d elements, model expects %d' % (name, src.numel(), dst.numel()))
            dst.copy_(src.to(dst.device))
        self.global_step = int(sd.get('global_step', 0))
        self._dirty = True
