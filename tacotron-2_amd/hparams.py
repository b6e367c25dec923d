"""Hyper-parameters of the MI355X WaveNet-vocoder tree: same key names and defaults as the reference's
hparams.py (its WaveNet + audio keys are the ones this tree reads; the Tacotron-only keys are accepted
so that `--hparams` strings written for the reference still parse, but nothing here consumes them).

Use ``hparams.parse("key=value,...")`` exactly as with the reference (train.py:35).
Extra keys of this tree are prefixed ``mi355_``.
"""
import math

from hparams_core import HParams

# ---- audio front-end keys read by the WaveNet path (reference hparams.py:63-116)
AUDIO = dict(
    num_mels=80, num_freq=1025, rescale=True, rescaling_max=0.999,
    clip_mels_length=True, max_mel_frames=900,
    use_lws=False, silence_threshold=2,
    n_fft=2048, hop_size=275, win_size=1100, sample_rate=22050, frame_shift_ms=None,
    magnitude_power=2.,
    trim_silence=True, trim_fft_size=2048, trim_hop_size=512, trim_top_db=40,
    signal_normalization=True, allow_clipping_in_normalization=True, symmetric_mels=True, max_abs_value=4.,
    normalize_for_wavenet=True, clip_for_wavenet=True, wavenet_pad_sides=1,
    preemphasize=True, preemphasis=0.97,
    min_level_db=-100, ref_level_db=20, fmin=55, fmax=7600,
    power=1.5, griffin_lim_iters=60, GL_on_GPU=True,
)

# ---- WaveNet model (reference hparams.py:187-233)
WAVENET_MODEL = dict(
    input_type='raw', quantize_channels=2 ** 16, use_bias=True, legacy=True, residual_legacy=True,
    log_scale_min=float(math.log(1e-14)), log_scale_min_gauss=float(math.log(1e-7)), cdf_loss=False,
    out_channels=2, layers=20, stacks=2, residual_channels=128, gate_channels=256, skip_out_channels=128,
    kernel_size=3,
    cin_channels=80, upsample_type='SubPixel', upsample_activation='Relu', upsample_scales=[11, 25],
    freq_axis_kernel_size=3, leaky_alpha=0.4, NN_init=True, NN_scaler=0.3,
    gin_channels=-1, use_speaker_embedding=True, n_speakers=5, speakers_path=None,
    speakers=['speaker0', 'speaker1', 'speaker2', 'speaker3', 'speaker4'],
)

# ---- WaveNet training / evaluation (reference hparams.py:294-338, 369-372)
WAVENET_TRAIN = dict(
    wavenet_random_seed=5339, wavenet_data_random_state=1234, wavenet_swap_with_cpu=False,
    wavenet_batch_size=8, wavenet_synthesis_batch_size=10 * 2, wavenet_test_size=None, wavenet_test_batches=1,
    wavenet_lr_schedule='exponential', wavenet_learning_rate=1e-3, wavenet_warmup=float(4000),
    wavenet_decay_rate=0.5, wavenet_decay_steps=200000,
    wavenet_adam_beta1=0.9, wavenet_adam_beta2=0.999, wavenet_adam_epsilon=1e-6,
    wavenet_clip_gradients=True, wavenet_ema_decay=0.9999, wavenet_weight_normalization=False,
    wavenet_init_scale=1., wavenet_dropout=0.05, wavenet_gradient_max_norm=100.0, wavenet_gradient_max_value=5.0,
    max_time_sec=None, max_time_steps=11000, wavenet_natural_eval=False, train_with_GTA=True,
    wavenet_synth_debug=False,
    wavenet_debug_wavs=['training_data/audio/audio-LJ001-0008.npy'],
    wavenet_debug_mels=['training_data/mels/mel-LJ001-0008.npy'],
)

HARDWARE = dict(cleaners='english_cleaners', tacotron_num_gpus=1, wavenet_num_gpus=1, split_on_cpu=True)

# ---- keys only the (out-of-scope) Tacotron feature-prediction model reads; accepted, never consumed here
TACOTRON_ONLY = dict(
    outputs_per_step=1, stop_at_any=True, batch_norm_position='after', clip_outputs=True, lower_bound_decay=0.1,
    embedding_dim=512, enc_conv_num_layers=3, enc_conv_kernel_size=(5,), enc_conv_channels=512, encoder_lstm_units=256,
    smoothing=False, attention_dim=128, attention_filters=32, attention_kernel=(31,), cumulative_weights=True,
    synthesis_constraint=False, synthesis_constraint_type='window', attention_win_size=7,
    prenet_layers=[256, 256], decoder_layers=2, decoder_lstm_units=1024, max_iters=10000,
    postnet_num_layers=5, postnet_kernel_size=(5,), postnet_channels=512,
    cbhg_kernels=8, cbhg_conv_channels=128, cbhg_pool_size=2, cbhg_projection=256, cbhg_projection_kernel_size=3,
    cbhg_highwaynet_layers=4, cbhg_highway_units=128, cbhg_rnn_units=128,
    mask_encoder=True, mask_decoder=False, cross_entropy_pos_weight=1, predict_linear=True,
    tacotron_random_seed=5339, tacotron_data_random_state=1234, tacotron_swap_with_cpu=False,
    tacotron_batch_size=32, tacotron_synthesis_batch_size=1, tacotron_test_size=0.05, tacotron_test_batches=None,
    tacotron_decay_learning_rate=True, tacotron_start_decay=40000, tacotron_decay_steps=18000, tacotron_decay_rate=0.5,
    tacotron_initial_learning_rate=1e-3, tacotron_final_learning_rate=1e-4,
    tacotron_adam_beta1=0.9, tacotron_adam_beta2=0.999, tacotron_adam_epsilon=1e-6,
    tacotron_reg_weight=1e-6, tacotron_scale_regularization=False, tacotron_zoneout_rate=0.1, tacotron_dropout_rate=0.5,
    tacotron_clip_gradients=True, tacotron_natural_eval=False,
    tacotron_teacher_forcing_mode='constant', tacotron_teacher_forcing_ratio=1., tacotron_teacher_forcing_init_ratio=1.,
    tacotron_teacher_forcing_final_ratio=0., tacotron_teacher_forcing_start_decay=10000,
    tacotron_teacher_forcing_decay_steps=40000, tacotron_teacher_forcing_decay_alpha=None, tacotron_fine_tuning=False,
    sentences=['Scientists at the CERN laboratory say they have discovered a new particle.'],
)

# ---- keys added by this tree
MI355 = dict(
    mi355_synthesis_chunk_frames=0,    # > 0: WaveNet.incremental (and so synthesize.py) generates through a stream, pushing this many mel frames at a
                                       # time (same samples, bit for bit); 0: one call for the whole utterance
    mi355_synthesis_temperature=1.0,   # sampling temperature of synthesis, in [0, 2]: scales the logistic / normal draw of the scalar heads, the class choice of the
                                       # softmax head; 0.6 ... 0.9 lowers the noise floor of a sampled vocoder, 0 is the deterministic decode (WaveNet.incremental(temperature=))
    mi355_synthesis_mixture_temperature=1.0,   # mixture-of-logistics head only: temperature of the component choice, in [0, 2] (0: the arg-max component)
    mi355_synthesis_slots=0,           # N > 0: Synthesizer.synthesize sends all utterances of a call through ONE slot session of min(N, 32) slots (continuous
                                       # batching: no padding to the longest utterance; tick = mi355_synthesis_chunk_frames or 8 frames); 0: padded batches
    mi355_synthesis_fold_rows=0,       # N > 0: Synthesizer.synthesize generates through WaveNet.folded: every utterance is cut into overlapping segments that run side by
                                       # side as up to min(N, 32) rows of one batch and are cross-faded back (groups of utterances whose rows fit 32); 0: off.
                                       # Not with mi355_synthesis_slots.  Segments start cold: the waveform is not the one-shot run's after the first seam
    mi355_synthesis_wide_rows=0,       # N > 0: Synthesizer.synthesize generates through WaveNet.wide: launch-per-layer runs of up to N utterances, N may exceed 32
                                       # (offline throughput: an evaluation set, GTA outputs); longest first, every run padded to its own longest.  0: off.
                                       # Not with mi355_synthesis_slots or mi355_synthesis_fold_rows
    mi355_synthesis_wide_slots=0,      # N > 0: Synthesizer.synthesize sends all utterances of a call through ONE wide slot session (WaveNet.wide_slots) of
                                       # min(N, utterances) slots, N may exceed 32: continuous batching on the launch-per-layer path, conditioning memory bounded by one
                                       # push (tick = mi355_synthesis_chunk_frames or 8 frames).  0: off.  Not with the three route keys above
    mi355_synthesis_fold_warm=4,       # mel frames a segment generates and discards before the part it contributes (50 ms at hop 275)
    mi355_synthesis_fold_fade=2,       # mel frames of cross-fade between consecutive segments (25 ms); equal power
    mi355_synthesis_fold_min_frames=40,    # no segment contributes fewer new frames than this (~0.5 s): shorter utterances stay one row, i.e. the one-shot run.
                                       # These three follow WaveRNN practice (11 000 / 550 samples); they have not been tuned by ear on a trained model of this tree
    mi355_output_deemphasis=False,     # True: the wavs Synthesizer writes are de-emphasised with hparams.preemphasis (the inverse of the preprocessing's pre-emphasis,
                                       # which the reference's save_wavenet_wav accepts and ignores); False: written as generated, as the reference writes them
    mi355_output_stage='host',         # 'host': audio.inv_preemphasis + save_wavenet_wav on numpy; 'device': decode, de-emphasis, peak normalisation and the int16
                                       # cast on the device (csrc/wn_post.hip, OutputStage.finish) on every synthesis route; the same files without de-emphasis
    mi355_output_gain=1.0,             # gain of the playable chunks of streams and slot sessions (WaveNet.output_stage): PCM = y * gain * 32767, clamped
    mi355_output_denoise=0.0,          # strength of the spectral bias denoiser (csrc/wn_denoise.hip) between the decode and the output stage of every route of
                                       # Synthesizer.synthesize and on eval_step's item: strength x the model's noise profile is subtracted from the magnitude of every STFT bin, the phase kept.  The
                                       # profile is fitted once at Synthesizer.load from what the model generates on silent conditioning.  0: no handle is created, nothing of
                                       # it runs and every file is byte-identical to a run without the key.  Not judged by ear: no trained checkpoint of this tree exists
    mi355_output_denoise_fft=1024,     # its window and transform length (periodic Hann); a multiple of 32, at most 4096
    mi355_output_denoise_hop=256,      # its hop, 1 ... fft / 4
    mi355_output_denoise_profile_frames=64,    # mel frames generated from silent conditioning for the profile (0.8 s at hop 275); at least fft samples
    mi355_output_denoise_speaker=0,    # the speaker id of that run on a globally conditioned model (one profile for all speakers)
    mi355_reconstruction_check=False,  # True: every utterance Synthesizer.synthesize generates (all three routes) and the item eval_step generates is analysed as preprocessing
                                       # analyses a recording and compared with its conditioning on the device (csrc/wn_melcmp.hip): one row per utterance appended to
                                       # wavs/reconstruction.tsv, one log line, two scalars beside the eval loss.  The wavs, map.txt and plots are byte-identical either way
    mi355_reconstruction_alarm_db=6.0, # a frame whose level-compensated mean |difference| exceeds this counts as alarmed.  A guess: nobody has a trained checkpoint of this tree,
                                       # so what a good model scores is unknown; set it from the clean score of your own model
    mi355_pitch_check=False,           # True: where ground-truth audio exists -- the item eval_step generates next to its target, synthesize.py --wavs_dir next to the
                                       # recordings (all three routes) -- F0 and voicing of both are estimated on the device (YIN, csrc/wn_pitch.hip) and compared: three
                                       # scalars beside the eval loss, one row per utterance appended to wavs/pitch.tsv, one log line.  False: nothing of it runs and every
                                       # file is byte-identical to a run without the key
    mi355_griffin_lim_baseline=False,  # True: beside every wav Synthesizer.synthesize writes (all three routes), wavs/griffin-lim-<basename>.wav: the model-free inversion of the
                                       # same conditioning (pinv of the mel filters, ** power, griffin_lim_iters iterations on the device, csrc/wn_griffin.hip; GL_on_GPU=False:
                                       # in numpy), and, with the two checks above on, its scores through the same check handles in wavs/reconstruction_griffin_lim.tsv /
                                       # wavs/pitch_griffin_lim.tsv with one log line beside the model's.  False: no handle exists, nothing of it runs and every file is
                                       # byte-identical to a run without the key
    mi355_alignment_reference_dir='',  # a directory of recordings: every utterance Synthesizer.synthesize generates (all three routes; the point is --mels_dir with PREDICTED
                                       # mels, whose output has another length and timing than any recording) whose basename -- as it is, or without a leading mel- --
                                       # has a <name>.wav there is aligned with it by dynamic time warping over the mel cepstra on the device (csrc/wn_align.hip) and scored
                                       # along the path: MCD-DTW, F0 RMSE, voicing and gross pitch error, one row appended to wavs/alignment.tsv, one log line.  '': no
                                       # handle exists, nothing of it runs and every file is byte-identical to a run without the key
    mi355_alignment_band=0,            # 0: every frame pair is admissible; r >= 1: only pairs with |i Fb - j Fa| <= r max(Fa, Fb)
    mi355_pitch_fmin=60.0,             # lowest f0 searched, Hz: tau_max = ceil(sample_rate / fmin)
    mi355_pitch_fmax=500.0,            # highest f0 searched, Hz: tau_min = max(2, sample_rate // fmax)
    mi355_pitch_threshold=0.15,        # YIN's absolute threshold on the normalised difference: a frame with no lag below it is unvoiced
    mi355_pitch_window=1024,           # terms of the difference function (46 ms at 22.05 kHz: 2.8 periods of 60 Hz)
    mi355_steps_per_graph=0,       # synthesis path: 0 = the persistent dataflow pipeline (real time at 22.05 kHz) whenever the model fits it, else the
                                   # launch-per-layer path with 32 steps per hipGraph replay; N > 0 = that path with N steps per replay
    mi355_synthetic_data=False,    # train on LJSpeech-shaped synthetic tensors (no dataset on disk)
    mi355_validation_interval=0,   # N > 0: every N training steps every rank scores its slice of the test split in batched dropout-free forwards
                                   # (WaveNet.validate: held-out negative log-likelihood per sample, training definition of the loss); 0: off
    mi355_train_stats=False,       # True: at every step that writes a summary rank 0 also writes what the reference's add_train_stats writes (train.py:41-56): per-tensor
                                   # gradient norms (wavenet_events/gradient_norms.jsonl), histograms of the decoded outputs, the targets, the Gaussian head's means and
                                   # log-scales and of the gradient norms (histograms.jsonl), and max / global gradient norm scalars, all reduced on the device
                                   # (csrc/wn_stats.hip).  False: every file is byte-identical to a run without the key, and nothing of it runs
    mi355_grad_buckets=3,        # data-parallel training: pieces of the flat gradient that are all-reduced while the backward is still running
    mi355_synthesize_with_ema=False,   # Synthesizer.load: pack the EMA shadow weights instead of the raw ones
    mi355_compute_dtype='bf16',     # 'bf16': bf16 MFMA operands, fp32 accumulation (the tuned path); 'fp32': the reference's own fp32 arithmetic for the
                                     # forward, loss AND backward (csrc/wn_f32.hip; ~13x slower: validation of a run against the reference's numerics) and
                                     # for synthesis (csrc/wn_synth_f32.hip: fp32 weights and queues like WaveNet.incremental; far from real time)
    mi355_device_mel=False,         # mel analysis on the GPU (csrc/wn_mel.hip).  wavenet_preprocess.py turns it on unless --hparams says otherwise (False: the
                                     # numpy float64 path, datasets.audio.melspectrogram); synthesize.py --wavs_dir always analyses on the device
    mi355_resample_input=False,     # True: wavenet_preprocess.py and synthesize.py --wavs_dir accept wavs of any sample rate: the parent converts the off-rate files to
                                     # sample_rate (csrc/wn_resample.hip in batches, one handle per rate; datasets.audio.resample_host with the same bits where no GPU
                                     # exists) before the host steps.  A Kaiser-windowed sinc with resampy's kaiser_best design values: close to librosa's load(sr=...),
                                     # not equal to it.  False: a file at another rate is an error, as before; files at sample_rate never pass through the resampler
    mi355_output_sample_rate=0,     # N > 0: the wavs Synthesizer writes are converted to N Hz after the de-emphasis and before the peak normalisation and the int16
                                     # cast, on both mi355_output_stage settings and every route; the checks keep seeing the model-rate signal.  0: no handle is created,
                                     # nothing of it runs and every file is byte-identical to a run without the key
    mi355_synthesis_live_chunk_ms=0,   # N > 0: synthesize.py --wavs_dir reads every recording in chunks of N ms and analyses and generates it push by push
                                     # (wavenet_vocoder/live.py: csrc/wn_mel_stream.hip feeding a slot session; the rescale gain from a first chunked pass over the file, as
                                     # --gain peak); the wavs grow as they are generated.  0: nothing of this runs and every file is byte-identical to a run without the key
)


def _build(overrides=None):
    kv = {}
    for group in (HARDWARE, AUDIO, TACOTRON_ONLY, WAVENET_MODEL, WAVENET_TRAIN, MI355):
        for k, v in group.items():
            kv[k] = list(v) if isinstance(v, list) else v
    if overrides:
        for k, v in overrides.items():
            if k not in kv:
                raise KeyError(k)
            kv[k] = v
    return HParams(**kv)


hparams = _build()


def hparams_debug_string():
    values = hparams.values()
    hp = ['  %s: %s' % (name, values[name]) for name in sorted(values) if name != 'sentences']
    return 'Hyperparameters:\n' + '\n'.join(hp)
