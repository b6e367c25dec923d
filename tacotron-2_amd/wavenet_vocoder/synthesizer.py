"""Synthesis front-end: same class, methods, file names and mel preparation as the reference's
``wavenet_vocoder/synthesizer.py`` (load / synthesize), running the HIP Fast-WaveNet loop."""
import os

import numpy as np
import torch

from scipy.io import wavfile

from datasets.audio import get_hop_size, inv_preemphasis, melspectrogram, save_wavenet_wav
from infolog import log
from wavenet_vocoder import util
from wavenet_vocoder.models import create_model


def _interp(feats, in_range):
    return (feats - in_range[0]) / (in_range[1] - in_range[0])


def _pad_inputs(x, maxlen, _pad=0):
    return np.pad(x, [(0, maxlen - len(x)), (0, 0)], mode='constant', constant_values=_pad)


class Synthesizer(object):
    def load(self, checkpoint_path, hparams, model_name='WaveNet'):
        log('Constructing model: {}'.format(model_name))
        self._hparams = hparams
        self.local_conditions, self.global_conditions = self._check_conditions()
        self.synth_debug = bool(hparams.wavenet_synth_debug)
        self.model = create_model(model_name, hparams)
        self._state = None
        self._tf_prefix = None
        if checkpoint_path is not None:
            log('Loading checkpoint: {}'.format(checkpoint_path))
            if os.path.exists(checkpoint_path + '.index'):
                # a checkpoint written by the reference (TensorFlow tensor bundle): read by name once the layout is known
                self._tf_prefix = checkpoint_path
            else:
                self._state = torch.load(checkpoint_path, map_location='cpu')
        self._capacity = (0, 0)
        self._post_stages = {}
        self._recon = None
        self._pitch_chk = None
        self._align_chk = None            # mi355_alignment_reference_dir: the AlignmentCheck; with the key empty no handle exists and nothing of it runs
        self.pitch_references = None      # mi355_pitch_check: the recordings of the next synthesize() call (run_wav_synthesis sets them)
        self._denoiser = None             # mi355_output_denoise > 0: the fitted OutputDenoiser; at 0 no handle exists and nothing of it runs
        if self._denoise_strength() > 0.0:
            frames = int(getattr(hparams, 'mi355_output_denoise_profile_frames', 64))
            self._ensure_capacity(1, frames * get_hop_size(hparams))
            self._denoiser = self.model.denoiser(1, frames * get_hop_size(hparams)).fit_from_model()
            log('Output denoiser: profile fitted on {} frames of silent conditioning, strength {:g}'.format(frames, self._denoise_strength()))

    def _denoise_strength(self):
        s = float(getattr(self._hparams, 'mi355_output_denoise', 0.0))
        if not (s >= 0.0) or s == float('inf'):
            raise ValueError('mi355_output_denoise must be finite and >= 0 (got {!r})'.format(s))
        return s

    def _denoise(self, rows, lengths):
        """mi355_output_denoise > 0: the decoded float rows [B, pitch] on the device, the first lengths[b] samples of each denoised IN PLACE at the fitted
        profile (WaveNet.denoiser; a handle that is too small is replaced by a larger one that takes the profile over).  Between the decode and the output
        stage on every route; the checks score what this returns.  At 0 the rows come back untouched."""
        dn = self._denoiser
        if dn is None:
            return rows
        lengths = [int(n) for n in lengths]
        if dn.rows < len(lengths) or dn.max_samples < max(lengths):
            big = self.model.denoiser(max(len(lengths), dn.rows), max(max(lengths), dn.max_samples))
            big.profile = dn.profile
            dn.close()
            dn = self._denoiser = big
        return dn.apply(rows, lengths, self._denoise_strength(), out=rows)

    def _output_mode(self):
        """(device, k): whether the written wavs come from the device output stage (mi355_output_stage), and the de-emphasis coefficient they get
        (mi355_output_deemphasis: hparams.preemphasis when the data was pre-emphasised; 0: written as generated).  The coefficient is the float32 value
        the device filter multiplies by, on the host path too: the two paths then differ by rounding alone (0.97 as a double is 3e-8 away, which the
        recursion amplifies to more int16 flips than all of the float32 arithmetic causes)."""
        hparams = self._hparams
        stage = str(getattr(hparams, 'mi355_output_stage', 'host'))
        if stage not in ('host', 'device'):
            raise ValueError("mi355_output_stage must be 'host' or 'device' (got {!r})".format(stage))
        deem = bool(getattr(hparams, 'mi355_output_deemphasis', False)) and bool(hparams.preemphasize)
        return stage == 'device', (float(np.float32(hparams.preemphasis)) if deem else 0.0)

    def _output_rate(self):
        """mi355_output_sample_rate: the rate of the written wavs, or 0 (off: no handle exists and nothing of it runs)"""
        rate = int(getattr(self._hparams, 'mi355_output_sample_rate', 0) or 0)
        if rate < 0:
            raise ValueError('mi355_output_sample_rate must be >= 0 (got {!r})'.format(rate))
        return rate

    def _resample_device(self, wavs, rate):
        """De-emphasised float32 utterances at the model rate (host arrays) -> (float32, peak-normalised int16) per utterance at `rate`: one
        Resampler.run on the device (WaveNet.output_resampler, kept; replaced by a larger one when it is too small), then its raw tail stage's finish."""
        lens = [len(w) for w in wavs]
        rs = getattr(self, '_resampler', None)
        if rs is None or rs.sr_out != rate or rs.rows < len(wavs) or rs.max_in < max(lens):
            rows, cap = max(len(wavs), rs.rows if rs else 0), max(max(lens), rs.max_in if rs else 0, 1)
            if rs is not None:
                rs.close()
            rs = self._resampler = self.model.output_resampler(rows, cap, rate)
        host = np.zeros((len(wavs), max(max(lens), 1)), np.float32)
        for b, w in enumerate(wavs):
            host[b, :lens[b]] = np.asarray(w, np.float32)
        z, n_out = rs.run(torch.from_numpy(host).to(self.model.device), lens)
        y, q = rs.tail.finish(z, n_out)
        y, q = y.cpu().numpy(), q.cpu().numpy()
        return [y[b, :n] for b, n in enumerate(n_out)], [q[b, :n] for b, n in enumerate(n_out)]

    def _stage(self, rows, in_type, k):
        """The output stage of (in_type, k) with at least `rows` rows (kept: a stage is a handle with device state)."""
        st = self._post_stages.get((in_type, k))
        if st is None or st.rows < rows:
            if st is not None:
                st.close()
            st = self._post_stages[(in_type, k)] = self.model.output_stage(rows, in_type=in_type, deemphasis=k)
        return st

    def _finish_device(self, wav, lengths, k):
        """Decoded waveforms [B, pitch] on the device -> (de-emphasised float32, peak-normalised int16) per utterance on the host (OutputStage.finish)."""
        y, q = self._stage(int(wav.shape[0]), 'raw', k).finish(wav.float().contiguous(), lengths)
        y, q = y.cpu().numpy(), q.cpu().numpy()
        return [y[b, :n] for b, n in enumerate(lengths)], [q[b, :n] for b, n in enumerate(lengths)]

    def _reconstruction(self, decoded, generated_wavs, cond, lengths, basenames, out_dir):
        """mi355_reconstruction_check: every utterance of the call scored against its conditioning (WaveNet.reconstruction_check), one row each appended to
        <out_dir>/reconstruction.tsv and one log line.  decoded: the decoded model-domain samples [B, >= lengths[b] * hop] on the device (the device output
        stage's input), or None on the host path: then what is about to be written, generated_wavs, is uploaded.  cond: [B, Tc, num_mels], the
        conditioning as the analysis scales it (clipped, before normalize_for_wavenet).  Reads results only: nothing the call writes otherwise changes."""
        if not bool(getattr(self._hparams, 'mi355_reconstruction_check', False)):
            return None
        from wavenet_vocoder import reconstruction
        hop = get_hop_size(self._hparams)
        dev = self.model.device
        n = [int(f) * hop for f in lengths]
        if decoded is None:
            host = np.zeros((len(n), max(n)), np.float32)
            for b, w in enumerate(generated_wavs):
                host[b, :n[b]] = np.asarray(w, np.float32)[:n[b]]
            decoded = torch.from_numpy(host).to(dev)
        decoded = decoded.float().contiguous()
        chk = self._recon
        if chk is None or chk.rows < len(n) or chk.max_samples < max(n):
            if chk is not None:
                chk.close()
            chk = self._recon = self.model.reconstruction_check(max(len(n), chk.rows if chk else 0), max(max(n), chk.max_samples if chk else 0))
        table = chk.score(decoded, n, torch.from_numpy(np.ascontiguousarray(cond, dtype=np.float32)).to(dev), frames=list(lengths), c_channels_first=False)
        reconstruction.append_tsv(os.path.join(out_dir, 'reconstruction.tsv'), basenames, lengths, table)
        log(reconstruction.log_line(basenames, table))
        self._recon_table = table          # (the Griffin-Lim baseline's log line puts its own means beside these)
        return table

    def _pitch(self, decoded, generated_wavs, basenames, out_dir):
        """mi355_pitch_check with recordings at hand (self.pitch_references: one model-domain signal per utterance of the call): F0 and voicing of every
        generated utterance against its recording (WaveNet.pitch_check), one row each appended to <out_dir>/pitch.tsv and one log line.  decoded /
        generated_wavs as _reconstruction takes them.  Reads results only; a failure logs one line and never fails the run."""
        refs, self.pitch_references = getattr(self, 'pitch_references', None), None
        self._baseline_refs = refs          # (the Griffin-Lim baseline of the same call is scored against the same recordings)
        if refs is None or not bool(getattr(self._hparams, 'mi355_pitch_check', False)):
            return None
        try:
            from wavenet_vocoder import pitch
            if len(refs) != len(basenames):
                raise ValueError('{} recordings for {} utterances'.format(len(refs), len(basenames)))
            dev = self.model.device
            glen = [int(decoded.shape[1])] * len(refs) if decoded is not None else [len(w) for w in generated_wavs]
            n = [min(len(r), g) for r, g in zip(refs, glen)]
            ref = np.zeros((len(n), max(max(n), 1)), np.float32)
            for b, r in enumerate(refs):
                ref[b, :n[b]] = np.asarray(r, np.float32)[:n[b]]
            if decoded is None:
                host = np.zeros_like(ref)
                for b, w in enumerate(generated_wavs):
                    host[b, :n[b]] = np.asarray(w, np.float32)[:n[b]]
                decoded = torch.from_numpy(host).to(dev)
            chk = getattr(self, '_pitch_chk', None)
            if chk is None or chk.rows < len(n) or chk.max_samples < max(n):
                if chk is not None:
                    chk.close()
                chk = self._pitch_chk = self.model.pitch_check(max(len(n), chk.rows if chk else 0), max(max(n), chk.max_samples if chk else 0))
            table = chk.score(decoded, torch.from_numpy(ref).to(dev), n)
            pitch.append_tsv(os.path.join(out_dir, 'pitch.tsv'), basenames, table)
            log(pitch.log_line(basenames, table))
            self._pitch_table = table
            return table
        except Exception as e:
            log('pitch check skipped: {}'.format(e))
            return None

    def _alignment(self, decoded, generated_wavs, lengths, basenames, out_dir):
        """mi355_alignment_reference_dir: every generated utterance whose basename has a recording there (alignment.reference_for: <basename>.wav, else the
        same without a leading mel-) aligned with it by dynamic time warping and scored along the path (WaveNet.alignment_check), one row each appended to
        <out_dir>/alignment.tsv and one log line.  The recordings are pre-emphasised as preprocessing does, so that they stand beside the model-domain
        output.  decoded / generated_wavs as _reconstruction takes them; lengths: mel frames per utterance.  Reads results only; a failure logs one line
        and never fails the run."""
        ref_dir = str(getattr(self._hparams, 'mi355_alignment_reference_dir', '') or '')
        if not ref_dir:
            return None
        try:
            from wavenet_vocoder import alignment
            from wavenet_vocoder.synthesize import pitch_references
            hop = get_hop_size(self._hparams)
            found = [(b, alignment.reference_for(ref_dir, name)) for b, name in enumerate(basenames)]
            found = [(b, p) for b, p in found if p is not None]
            if not found:
                log('Alignment check: none of the {} utterance(s) has a recording in {}'.format(len(basenames), ref_dir))
                return None
            refs = pitch_references([p for _, p in found], self._hparams)
            names = [basenames[b] for b, _ in found]
            gl, rl = [int(lengths[b]) * hop for b, _ in found], [len(r) for r in refs]
            dev = self.model.device
            ref = np.zeros((len(refs), max(max(rl), 1)), np.float32)
            for k, r in enumerate(refs):
                ref[k, :rl[k]] = r
            if decoded is None:
                gen = np.zeros((len(found), max(gl)), np.float32)
                for k, (b, _) in enumerate(found):
                    gen[k, :gl[k]] = np.asarray(generated_wavs[b], np.float32)[:gl[k]]
                gen = torch.from_numpy(gen).to(dev)
            else:
                gen = decoded.float()[[b for b, _ in found]].contiguous()
            chk = self._align_chk
            need = max(max(gl), max(rl))
            if chk is None or chk.rows < len(found) or chk.max_samples < need:
                rows, cap = max(len(found), chk.rows if chk else 0), max(need, chk.max_samples if chk else 0)
                if chk is not None:
                    chk.close()
                chk = self._align_chk = self.model.alignment_check(rows, cap)
            table = chk.score(gen, gl, torch.from_numpy(ref).to(dev), rl)
            alignment.append_tsv(os.path.join(out_dir, 'alignment.tsv'), names, table)
            log(alignment.log_line(names, table))
            return table
        except Exception as e:
            log('alignment check skipped: {}'.format(e))
            return None

    def _griffin_lim_baseline(self, mel_spectrograms, basenames, out_dir):
        """mi355_griffin_lim_baseline: beside every generated wav, <out_dir>/griffin-lim-<basename>.wav -- the model-free inversion of the same conditioning
        (datasets.audio.inv_mel_spectrogram_device, csrc/wn_griffin.hip; with GL_on_GPU off the numpy path), hop (frames - 1) samples, de-emphasised when
        the generated wavs are (mi355_output_deemphasis).  With mi355_reconstruction_check / mi355_pitch_check on, the Griffin-Lim signal BEFORE the
        de-emphasis (the checks' model domain) is scored through the same check handles into <out_dir>/reconstruction_griffin_lim.tsv /
        pitch_griffin_lim.tsv, and one log line puts the batch means beside the model's.  Off: no handle exists and nothing runs.  A mel of one frame has
        no Griffin-Lim signal and is left out.  Reads results only: nothing the call writes otherwise changes."""
        hparams = self._hparams
        recon_table, self._recon_table = getattr(self, '_recon_table', None), None
        pitch_table, self._pitch_table = getattr(self, '_pitch_table', None), None
        refs, self._baseline_refs = getattr(self, '_baseline_refs', None), None
        if not bool(getattr(hparams, 'mi355_griffin_lim_baseline', False)):
            return None
        from datasets import audio
        keep = [b for b, m in enumerate(mel_spectrograms) if len(m) >= 2]
        if not keep:
            return []
        mels = [np.ascontiguousarray(np.asarray(mel_spectrograms[b], np.float32).T) for b in keep]
        names, frames = [basenames[b] for b in keep], [int(m.shape[1]) for m in mels]
        hop, seed = get_hop_size(hparams), int(getattr(hparams, 'wavenet_random_seed', 0))
        k = self._output_mode()[1]
        if bool(getattr(hparams, 'GL_on_GPU', True)):
            gl = getattr(self, '_griffin', None)
            if gl is None or gl.rows < min(len(mels), audio.GRIFFIN_BATCH) or gl.max_frames < max(frames):
                if gl is not None:
                    gl.close()
                gl = self._griffin = self.model.griffin_lim(max(min(len(mels), audio.GRIFFIN_BATCH), gl.rows if gl else 0), max(max(frames), gl.max_frames if gl else 0))
            _, raw = audio.inv_mel_spectrogram_device(mels, None, hparams, seed=seed, griffin=gl, deemphasize=False, return_model_domain=True)
        else:
            raw = audio.inv_mel_spectrogram_host(mels, hparams, seed=seed, deemphasize=False)
        paths = []
        for name, w in zip(names, raw):
            paths.append(os.path.join(out_dir, 'griffin-lim-{}.wav'.format(name)))
            save_wavenet_wav(inv_preemphasis(w, k).astype(np.float32) if k != 0.0 else w, paths[-1], sr=hparams.sample_rate)
        n = [len(w) for w in raw]
        parts = []
        if bool(getattr(hparams, 'mi355_reconstruction_check', False)) or (bool(getattr(hparams, 'mi355_pitch_check', False)) and refs is not None):
            dev = self.model.device
            host = np.zeros((len(n), max(n)), np.float32)
            for b, w in enumerate(raw):
                host[b, :n[b]] = w
            decoded = torch.from_numpy(host).to(dev)
        if bool(getattr(hparams, 'mi355_reconstruction_check', False)):
            from wavenet_vocoder import reconstruction
            lo = -hparams.max_abs_value if hparams.symmetric_mels else 0
            cond = np.stack([_pad_inputs(m.T, max(frames), _pad=lo) for m in mels]).astype(np.float32)
            chk = getattr(self, '_recon', None)
            if chk is None or chk.rows < len(n) or chk.max_samples < max(n):
                if chk is not None:
                    chk.close()
                chk = self._recon = self.model.reconstruction_check(max(len(n), chk.rows if chk else 0), max(max(n), chk.max_samples if chk else 0))
            table = chk.score(decoded, n, torch.from_numpy(cond).to(dev), frames=frames, c_channels_first=False)
            reconstruction.append_tsv(os.path.join(out_dir, 'reconstruction_griffin_lim.tsv'), names, frames, table)
            t = np.asarray(table, np.float64).reshape(len(n), -1)
            parts.append('reconstruction l1c {:.2f} dB, lsdc {:.2f} dB, mcd {:.2f} dB'.format(t[:, 4].mean(), t[:, 5].mean(), t[:, 3].mean()) +
                         (' (model {:.2f} / {:.2f} / {:.2f})'.format(*[np.asarray(recon_table, np.float64)[:, c].mean() for c in (4, 5, 3)]) if recon_table is not None else ''))
        if bool(getattr(hparams, 'mi355_pitch_check', False)) and refs is not None:
            try:
                from wavenet_vocoder import pitch
                if len(refs) != len(basenames):
                    raise ValueError('{} recordings for {} utterances'.format(len(refs), len(basenames)))
                refs = [refs[b] for b in keep]
                m = [min(len(r), g) for r, g in zip(refs, n)]
                ref = np.zeros((len(m), max(max(m), 1)), np.float32)
                for b, r in enumerate(refs):
                    ref[b, :m[b]] = np.asarray(r, np.float32)[:m[b]]
                chk = getattr(self, '_pitch_chk', None)
                if chk is None or chk.rows < len(m) or chk.max_samples < max(m):
                    if chk is not None:
                        chk.close()
                    chk = self._pitch_chk = self.model.pitch_check(max(len(m), chk.rows if chk else 0), max(max(m), chk.max_samples if chk else 0))
                table = chk.score(decoded, torch.from_numpy(ref).to(dev), m)
                pitch.append_tsv(os.path.join(out_dir, 'pitch_griffin_lim.tsv'), names, table)
                t = np.asarray(table, np.float64).reshape(len(m), -1)
                parts.append('pitch V/UV error {:.3f}, gross pitch error {:.3f}, F0 RMSE {:.1f} cents'.format(t[:, 4].mean(), t[:, 5].mean(), t[:, 6].mean()) +
                             (' (model {:.3f} / {:.3f} / {:.1f})'.format(*[np.asarray(pitch_table, np.float64)[:, c].mean() for c in (4, 5, 6)]) if pitch_table is not None else ''))
            except Exception as e:
                log('pitch check of the Griffin-Lim baseline skipped: {}'.format(e))
        log('Griffin-Lim baseline: {} utterance(s), {} iterations'.format(len(names), int(hparams.griffin_lim_iters)) + ''.join('; ' + p for p in parts))
        return paths

    def _ensure_capacity(self, batch, time_steps):
        if batch <= self._capacity[0] and time_steps <= self._capacity[1]:
            return
        if self.model.engine is not None:
            self.model.engine.close()
            self.model.engine = None
        cap = (max(batch, self._capacity[0]), max(time_steps, self._capacity[1]))
        # synthesis-only engine: no saved-activation / backward workspace (that is ~45 KB of HBM per (stream x sample) at the paper
        # shape, i.e. ~180 GB for the default 20 x 9 s batch; what synthesis needs is ~1.5 KB) and every buffer pre-sized
        self.model.build(cap[0], cap[1], inference_only=True)
        if self._tf_prefix is not None:
            from wavenet_vocoder.tf_checkpoint import load_reference_checkpoint
            flat, step, missing = load_reference_checkpoint(self._tf_prefix, self.model.engine.layout)
            if missing:
                raise RuntimeError('TensorFlow checkpoint {} lacks {} of the model\'s tensors, e.g. {}'.format(self._tf_prefix, len(missing), missing[:3]))
            p = torch.from_numpy(flat)
            self._state = {'params': p, 'ema': p.clone(), 'adam_m': torch.zeros_like(p), 'adam_v': torch.zeros_like(p), 'global_step': step or 0}
            self._tf_prefix = None
        if self._state is not None:
            self.model.load_state_dict(self._state)
            self.model.use_ema_weights() if getattr(self._hparams, 'mi355_synthesize_with_ema', False) else None
        self._capacity = (cap[0], self.model.max_time)

    def synthesize(self, mel_spectrograms, speaker_ids, basenames, out_dir, log_dir):
        hparams = self._hparams
        if self.synth_debug:
            assert len(hparams.wavenet_debug_mels) == len(hparams.wavenet_debug_wavs)
            mel_spectrograms = [np.load(mel_file) for mel_file in hparams.wavenet_debug_mels]
        hop = get_hop_size(hparams)
        audio_lengths = [len(x) * hop for x in mel_spectrograms]
        maxlen = max(len(x) for x in mel_spectrograms)
        T2_output_range = (-hparams.max_abs_value, hparams.max_abs_value) if hparams.symmetric_mels else (0, hparams.max_abs_value)
        if hparams.clip_for_wavenet:
            mel_spectrograms = [np.clip(x, T2_output_range[0], T2_output_range[1]) for x in mel_spectrograms]
        c_batch = np.stack([_pad_inputs(x, maxlen, _pad=T2_output_range[0]) for x in mel_spectrograms]).astype(np.float32)
        cond, frames = c_batch, [len(x) for x in mel_spectrograms]          # the conditioning in the analysis' own scale: what a reconstruction check compares with
        if hparams.normalize_for_wavenet:
            c_batch = _interp(c_batch, T2_output_range).astype(np.float32)
        # global condition: int32 speaker ids [B, 1] (reference synthesizer.py:72)
        g = None
        if self.global_conditions:
            if speaker_ids is None:
                raise RuntimeError('Please provide speaker ids (--speaker_id) to a globally conditioned WaveNet')
            g = torch.from_numpy(np.asarray(speaker_ids, dtype=np.int32).reshape(len(c_batch), 1))
        nfold = int(getattr(hparams, 'mi355_synthesis_fold_rows', 0))
        nwide = int(getattr(hparams, 'mi355_synthesis_wide_rows', 0))
        routes = [key for key in ('mi355_synthesis_fold_rows', 'mi355_synthesis_slots', 'mi355_synthesis_wide_rows', 'mi355_synthesis_wide_slots')
                  if int(getattr(hparams, key, 0)) > 0]
        if len(routes) > 1:
            raise ValueError('{} are {} > 0: choose one'.format(' and '.join(routes), 'both' if len(routes) == 2 else 'all'))
        if nwide > 0 and not self.synth_debug:
            generated_wavs, upsampled_features, pcm, decoded = self._synthesize_wide(c_batch, frames, speaker_ids, nwide)
            self._reconstruction(decoded, generated_wavs, cond, frames, basenames, out_dir)
            self._pitch(decoded, generated_wavs, basenames, out_dir)
            self._alignment(decoded, generated_wavs, frames, basenames, out_dir)
            return self._write(generated_wavs, upsampled_features, mel_spectrograms, basenames, out_dir, log_dir, pcm)
        if nfold > 0 and not self.synth_debug:
            generated_wavs, upsampled_features, pcm, decoded = self._synthesize_folded(c_batch, frames, speaker_ids, min(nfold, 32), log_dir is not None)
            self._reconstruction(decoded, generated_wavs, cond, frames, basenames, out_dir)
            self._pitch(decoded, generated_wavs, basenames, out_dir)
            self._alignment(decoded, generated_wavs, frames, basenames, out_dir)
            return self._write(generated_wavs, upsampled_features, mel_spectrograms, basenames, out_dir, log_dir, pcm)
        nslots, nwslots = int(getattr(hparams, 'mi355_synthesis_slots', 0)), int(getattr(hparams, 'mi355_synthesis_wide_slots', 0))
        if (nslots > 0 or nwslots > 0) and not self.synth_debug:
            generated_wavs, upsampled_features, pcm, decoded = self._synthesize_slots(c_batch, frames, speaker_ids, nwslots if nwslots > 0 else min(nslots, 32),
                                                                                      log_dir is not None, wide=nwslots > 0)
            self._reconstruction(decoded, generated_wavs, cond, frames, basenames, out_dir)
            self._pitch(decoded, generated_wavs, basenames, out_dir)
            self._alignment(decoded, generated_wavs, frames, basenames, out_dir)
            return self._write(generated_wavs, upsampled_features, mel_spectrograms, basenames, out_dir, log_dir, pcm)
        self._ensure_capacity(len(c_batch), maxlen * hop)
        dev = self.model.device
        test_inputs = None
        if self.synth_debug:
            test_wavs = [np.load(w).reshape(-1) for w in hparams.wavenet_debug_wavs]
            T = maxlen * hop
            test_inputs = torch.from_numpy(np.stack([np.pad(w[:T], (0, max(0, T - len(w)))) for w in test_wavs]).astype(np.float32)).to(dev)
        # c: [B, Tc, num_mels] like the reference's placeholder; the model transposes it (wavenet.py:427)
        self.model.initialize(None, torch.from_numpy(c_batch).to(dev), None if g is None else g.to(dev), None, test_inputs=test_inputs)
        torch.cuda.synchronize()
        self.model.engine.synth_check()           # the generation is enqueued asynchronously: a pipeline hand-off timeout surfaces here
        device, k = self._output_mode()
        pcm = None
        y_hat = self.model.tower_y_hat[0]
        if self._denoiser is not None and not self.synth_debug:
            y_hat = self._denoise(y_hat.float().contiguous().clone(), audio_lengths)
        if device:
            generated_wavs, pcm = self._finish_device(y_hat, audio_lengths, k)
        else:
            generated = y_hat.float().cpu().numpy()
            generated_wavs = [w[:length] for w, length in zip(generated, audio_lengths)]
        feats = self.model.tower_synth_upsampled_local_features[0].cpu().numpy()
        upsampled_features = [f[:, :length] for f, length in zip(feats, audio_lengths)]
        if not self.synth_debug:
            self._reconstruction(y_hat if device else None, generated_wavs, cond, frames, basenames, out_dir)
            self._pitch(y_hat if device else None, generated_wavs, basenames, out_dir)
            self._alignment(y_hat if device else None, generated_wavs, frames, basenames, out_dir)
        return self._write(generated_wavs, upsampled_features, mel_spectrograms, basenames, out_dir, log_dir, pcm)

    def _synthesize_folded(self, c_batch, lengths, speaker_ids, nrows, want_features):
        """mi355_synthesis_fold_rows > 0: the utterances of the call through WaveNet.folded, in groups of consecutive utterances whose rows fit nrows (every
        utterance takes at least one row, so at most nrows utterances per group).  Seeds derive from (wavenet_random_seed, the model's synthesis-call
        counter), so two fresh runs of the same inputs agree."""
        from wavenet_vocoder import _ext
        from wavenet_vocoder.models.wavenet import fold_capacity, unfold_features
        hparams, hop = self._hparams, get_hop_size(self._hparams)
        warm, fade = int(hparams.mi355_synthesis_fold_warm), int(hparams.mi355_synthesis_fold_fade)
        min_keep = int(hparams.mi355_synthesis_fold_min_frames)
        groups = [list(range(u0, min(u0 + nrows, len(lengths)))) for u0 in range(0, len(lengths), nrows)]
        plans = [_ext.fold_plan([lengths[u] for u in grp], nrows, warm, fade, min_keep) for grp in groups]
        caps = [fold_capacity([lengths[u] for u in grp], plan, hop) for grp, plan in zip(groups, plans)]
        self._ensure_capacity(max(c[0] for c in caps), max(c[1] for c in caps))
        wavs, ups = [], []
        device, k = self._output_mode()
        dn = self._denoiser is not None
        staged = device and not dn          # the fold's own stage finishes every group; with the denoiser on, the rows are denoised and finished after the loop, as a whole
        pcm = [] if staged else None
        check = device and (bool(getattr(hparams, 'mi355_reconstruction_check', False)) or
                            (bool(getattr(hparams, 'mi355_pitch_check', False)) and getattr(self, 'pitch_references', None) is not None) or
                            bool(getattr(hparams, 'mi355_alignment_reference_dir', '')))
        keep = check or dn
        decoded = torch.zeros(len(lengths), max(lengths) * hop, device=self.model.device) if keep else None      # out_wav of every group, kept on the device
        ids = None if not self.global_conditions else np.asarray(speaker_ids).reshape(-1)
        for grp, plan in zip(groups, plans):
            cl = [torch.from_numpy(np.ascontiguousarray(c_batch[u, :lengths[u]].T)) for u in grp]
            res = self.model.folded(cl, g=None if ids is None else [int(ids[u]) for u in grp], rows=plan, check=True, return_rows=want_features,
                                    post=self._stage(len(grp), 'raw', k) if staged else None)
            if staged:          # the written waveform is the stage's: de-emphasised float32 for the plots, int16 for the file
                posts = res[-1]
                res = res[0] if len(res) == 2 else res[:2]
                pcm += [q.cpu().numpy() for _, q in posts]
            if keep:
                for u, w in zip(grp, res[0] if want_features else res):
                    decoded[u, :w.shape[0]] = w
            if want_features:
                res, info = res
                ups += [f.cpu().numpy() for f in unfold_features(plan, info['features'], hop)]
            else:
                ups += [np.zeros((hparams.cin_channels, 0), np.float32) for _ in grp]
            if not dn:
                wavs += [w.float().cpu().numpy() for w in ([y for y, _ in posts] if staged else res)]
        if dn:          # decode (the fold's), denoise, output stage
            n = [f * hop for f in lengths]
            decoded = self._denoise(decoded, n)
            if device:
                wavs, pcm = self._finish_device(decoded, n, k)
            else:
                host = decoded.cpu().numpy()
                wavs, decoded = [host[u, :n[u]] for u in range(len(n))], None
        return wavs, ups, pcm, decoded

    def _synthesize_wide(self, c_batch, lengths, speaker_ids, nrows):
        """mi355_synthesis_wide_rows > 0: the utterances of the call through WaveNet.wide, in launch-per-layer runs of at most nrows utterances (nrows may
        exceed 32), longest first, every run padded to its own longest utterance; results in input order.  The inference-only context is built for the
        largest run.  Seeds derive from (wavenet_random_seed, the model's synthesis-call counter, run index), so two fresh runs of the same inputs agree."""
        from wavenet_vocoder import util as wutil
        from wavenet_vocoder.models.wavenet import wide_plan
        from wavenet_vocoder.util import is_mulaw, is_mulaw_quantize
        hparams, hop = self._hparams, get_hop_size(self._hparams)
        runs, _ = wide_plan(lengths, nrows, nrows * max(lengths))
        self._ensure_capacity(max(len(r) for r in runs), max(lengths) * hop)
        m = self.model
        dev = m.device
        cl = [torch.from_numpy(np.ascontiguousarray(c_batch[u, :lengths[u]].T)) for u in range(len(lengths))]
        ids = None if not self.global_conditions else [int(v) for v in np.asarray(speaker_ids).reshape(-1)]
        samples, info = m.wide(cl, g=ids, rows=nrows, check=True)
        device, k = self._output_mode()
        rows = torch.zeros(len(lengths), max(lengths) * hop, device=dev)      # every utterance decoded, one row each
        for u, out in enumerate(samples):
            if is_mulaw_quantize(hparams.input_type):
                out = wutil.inv_mulaw_quantize(out)
            elif is_mulaw(hparams.input_type):
                out = wutil.inv_mulaw(out)
            rows[u, :out.shape[0]] = out.float()
        ups = [f.cpu().numpy() for f in info['features']]
        rows = self._denoise(rows, [n * hop for n in lengths])
        if device:
            wavs, pcm = self._finish_device(rows, [n * hop for n in lengths], k)
            return wavs, ups, pcm, rows
        host = rows.cpu().numpy()
        return [host[u, :n * hop] for u, n in enumerate(lengths)], ups, None, None

    def _synthesize_slots(self, c_batch, lengths, speaker_ids, nslots, want_features, wide=False):
        """mi355_synthesis_slots > 0: all utterances of the call through ONE slot session (WaveNet.slots): no utterance is padded to the longest of its
        batch, a slot that finishes takes the next utterance at the next push.  Seeds derive from (wavenet_random_seed, the model's synthesis-call
        counter, utterance index), so two fresh runs of the same inputs agree, whatever the tick.  wide (mi355_synthesis_wide_slots > 0): the same
        through ONE wide session (WaveNet.wide_slots) of nslots slots, which may exceed 32."""
        from wavenet_vocoder.models.wavenet import slot_plan, temperature_pair
        from wavenet_vocoder import util as wutil
        from wavenet_vocoder.util import is_mulaw, is_mulaw_quantize
        hparams, hop = self._hparams, get_hop_size(self._hparams)
        tick = int(getattr(hparams, 'mi355_synthesis_chunk_frames', 0)) or 8
        B = min(nslots, len(lengths))
        self._ensure_capacity(B, (tick + 8) * hop)          # a push generates at most tick + lookahead frames per slot
        m = self.model
        dev = m.device
        right = m.engine.stream_lookahead()[1]
        if (tick + right) * hop > m.max_time:
            self._ensure_capacity(B, (tick + right) * hop)
        m._synth_calls = getattr(m, '_synth_calls', 0) + 1
        base = ((int(hparams.wavenet_random_seed) << 20) + m._synth_calls) << 20
        sess = m.wide_slots(B) if wide else m.slots(B)
        pair = temperature_pair(hparams)                  # every utterance is opened at the hparams temperature (SlotSession.open)
        if pair != (1.0, 1.0) and getattr(self, '_logged_temperature', None) != pair:
            self._logged_temperature = pair
            log('WaveNet synthesis slots: sampling temperature {:g}, choice temperature {:g}'.format(*pair))
        device, k = self._output_mode()
        decode = self._stage(B, hparams.input_type, 0.0) if device else None      # per push: the decode alone; the whole utterance is finished below
        chunks = [[] for _ in lengths]
        feats = [[] for _ in lengths]
        owner, sent = [None] * B, [0] * len(lengths)
        for opens, frames, final in slot_plan(lengths, B, tick):
            for b, u in opens:
                sess.open(b, g=None if not self.global_conditions else int(np.asarray(speaker_ids).reshape(-1)[u]), seed=base + u)
                owner[b] = u
            items = {}
            for b in range(B):
                if owner[b] is None:
                    continue
                u = owner[b]
                blk = torch.from_numpy(np.ascontiguousarray(c_batch[u, sent[u]:sent[u] + frames[b]].T))
                items[b] = (blk, final[b])
                sent[u] += frames[b]
            res = sess.push(items, post=decode, post_output='float')
            if device:
                res = {b: y for b, (_, y) in res.items()}
            fe = None
            if want_features:
                n_max = max(int(v.shape[0]) for v in res.values())
                if n_max > 0:
                    fe = torch.empty(B, hparams.cin_channels, n_max, device=dev)
                    m.engine.upsampled_features(fe)
            for b, smp in res.items():
                u = owner[b]
                chunks[u].append(smp.clone())
                if fe is not None and smp.shape[0] > 0:
                    feats[u].append(fe[b, :, :smp.shape[0]].clone())
                if final[b]:
                    owner[b] = None
        torch.cuda.synchronize()
        sess.check()
        sess.close()
        wavs, ups, pcm, rows = [], [], None, None
        if device:
            rows = torch.zeros(len(lengths), max(lengths) * hop, device=dev)
            for u, n in enumerate(lengths):
                if chunks[u]:
                    rows[u, :n * hop] = torch.cat(chunks[u])
            rows = self._denoise(rows, [n * hop for n in lengths])
            wavs, pcm = self._finish_device(rows, [n * hop for n in lengths], k)
        host_rows = torch.zeros(len(lengths), max(lengths) * hop, device=dev) if (self._denoiser is not None and not device) else None
        for u, n in enumerate(lengths):
            if not device:
                out = torch.cat(chunks[u]) if chunks[u] else torch.zeros(0, device=dev)
                assert out.shape[0] == n * hop, (u, out.shape, n * hop)
                if is_mulaw_quantize(hparams.input_type):
                    out = wutil.inv_mulaw_quantize(out)
                elif is_mulaw(hparams.input_type):
                    out = wutil.inv_mulaw(out)
                if host_rows is not None:
                    host_rows[u, :n * hop] = out.float()
                else:
                    wavs.append(out.float().cpu().numpy())
            ups.append(torch.cat(feats[u], 1).cpu().numpy() if feats[u] else np.zeros((hparams.cin_channels, 0), np.float32))
        if host_rows is not None:          # the decoded utterances of the call denoised together, in one call
            host = self._denoise(host_rows, [n * hop for n in lengths]).cpu().numpy()
            wavs = [host[u, :n * hop] for u, n in enumerate(lengths)]
        return wavs, ups, pcm, rows      # rows: every utterance's decoded chunks, kept on the device until it finished (None on the host path)

    def _write(self, generated_wavs, upsampled_features, mel_spectrograms, basenames, out_dir, log_dir, pcm=None):
        """pcm: the device output stage's int16 per utterance (mi355_output_stage = 'device': generated_wavs are its de-emphasised floats); None: the host path."""
        hparams = self._hparams
        k = self._output_mode()[1]
        audio_filenames = []
        rate, converted = self._output_rate(), None
        if rate > 0:      # after the de-emphasis (a filter designed at the model rate), before the peak normalisation and the int16 cast; the plots keep the model-rate signal
            if pcm is not None:
                converted = self._resample_device(generated_wavs, rate)[1]
            else:
                from datasets import audio
                deem = [inv_preemphasis(w, k).astype(np.float32) if k != 0.0 else np.asarray(w, np.float32) for w in generated_wavs]
                converted = audio.resample_signals(deem, hparams.sample_rate, rate)
        for i, (wav, feat, input_mel) in enumerate(zip(generated_wavs, upsampled_features, mel_spectrograms)):
            audio_filename = os.path.join(out_dir, 'wavenet-audio-{}.wav'.format(basenames[i]))
            if converted is not None and pcm is not None:
                wavfile.write(audio_filename, rate, converted[i])
            elif converted is not None:
                save_wavenet_wav(converted[i], audio_filename, sr=rate, inv_preemphasize=hparams.preemphasize, k=hparams.preemphasis)
            elif pcm is not None:
                wavfile.write(audio_filename, hparams.sample_rate, pcm[i])
            else:
                if k != 0.0:
                    wav = inv_preemphasis(wav, k).astype(np.float32)
                save_wavenet_wav(wav, audio_filename, sr=hparams.sample_rate, inv_preemphasize=hparams.preemphasize, k=hparams.preemphasis)
            audio_filenames.append(audio_filename)
            if log_dir is not None:
                try:
                    # generated-audio mel vs the conditioning mel (reference synthesizer.py:113-117)
                    util.plot_spectrogram(melspectrogram(wav.astype(np.float64), hparams).T,
                                          os.path.join(log_dir, 'wavenet-mel-spectrogram-{}.png'.format(basenames[i])),
                                          title='Local Condition vs Reconstructed Audio Mel-Spectrogram analysis', target_spectrogram=input_mel)
                    util.plot_spectrogram(feat.T, os.path.join(log_dir, 'wavenet-upsampled_features-{}.png'.format(basenames[i])),
                                          title='Upmsampled Local Condition features', auto_aspect=True)
                    util.waveplot(os.path.join(log_dir, 'wavenet-waveplot-{}.png'.format(basenames[i])), wav, None, hparams,
                                  title='WaveNet generated Waveform.')
                except Exception as e:
                    log('plotting skipped: {}'.format(e))
        self._griffin_lim_baseline(mel_spectrograms, basenames, out_dir)
        return audio_filenames

    def _check_conditions(self):
        return self._hparams.cin_channels > 0, self._hparams.gin_channels > 0
