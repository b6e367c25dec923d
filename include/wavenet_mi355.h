/*
 * wavenet_mi355.h -- C ABI of libwavenet_mi355.so: the MI355X (gfx950) native WaveNet-vocoder
 * training / Fast-WaveNet synthesis hot path.
 *
 * The reference (Rayhane-mamah/Tacotron-2) has NO native / FFI boundary: its hot path is a chain of
 * TensorFlow-1 graph ops built by the Python class wavenet_vocoder/models/wavenet.py:WaveNet and run
 * with session.run (wavenet_vocoder/train.py:303, synthesizer.py:97).  This header is therefore the
 * boundary the reference *would* bind if it had one; each entry point names the reference code whose
 * arithmetic it replaces.  The Python mirror of the reference's class API that calls these functions
 * through ctypes lives in tacotron-2_amd/wavenet_vocoder/ (see INTEGRATION.md).
 *
 * Conventions
 *   - every function returns an int status: 0 = WN_OK, negative = error; wn_last_error() gives text.
 *     No C++ exception crosses this boundary.
 *   - all data pointers are DEVICE pointers (HBM) owned by the caller and borrowed for the call only,
 *     unless the parameter is documented "host".  Tensors are contiguous in the stated layout.
 *   - all work is enqueued asynchronously, ordered after everything already on the caller's stream (`void* stream` is a
 *     hipStream_t) and before whatever the caller enqueues next (ctx-owned side streams are forked and joined with events);
 *     no entry point of the drop-in surface synchronises the device (wn_synth_check and the WN_TEST_HOOKS say so where they do).
 *     One wn_ctx per (process, device); not thread-safe.
 *   - memory: wn_create sizes the workspace once for (max_batch, max_time).  Training contexts allocate their synthesis state on the
 *     first wn_synthesize (eval steps); inference-only contexts (cfg.inference_only) pre-size it and never allocate afterwards.
 *   - parameters, gradients and optimiser slots are single flat fp32 buffers; the tensors inside them
 *     keep the reference's TensorFlow layouts ([k,in,out] conv kernels ...) at the offsets reported by
 *     wn_tensor_info(), under names mirroring the reference's variable scopes.
 */
#ifndef WAVENET_MI355_H
#define WAVENET_MI355_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WN_ABI_VERSION 4

enum wn_status {
    WN_OK = 0,
    WN_E_ARG = -1,          /* bad argument / null pointer            */
    WN_E_SHAPE = -2,        /* shape constraint violated              */
    WN_E_HIP = -3,          /* HIP runtime error (see wn_last_error)  */
    WN_E_UNSUPPORTED = -4,  /* valid reference config not built yet   */
    WN_E_STATE = -5         /* call order violated (e.g. bwd before fwd) */
};

enum wn_input_type { WN_INPUT_RAW = 0, WN_INPUT_MULAW = 1, WN_INPUT_MULAW_QUANTIZE = 2 }; /* hparams.py:187 */
enum wn_upsample_type {                                                                    /* hparams.py:219 */
    WN_UP_NEAREST = 0, WN_UP_2D = 1, WN_UP_SUBPIXEL = 2, WN_UP_1D = 3, WN_UP_RESIZE = 4
};
enum wn_activation { WN_ACT_NONE = 0, WN_ACT_RELU = 1, WN_ACT_LEAKY_RELU = 2 };             /* hparams.py:220 */
enum wn_lr_schedule { WN_LR_EXPONENTIAL = 0, WN_LR_NOAM = 1 };                              /* hparams.py:309 */
/* Arithmetic of training / the teacher-forced forward (WaveNet.step, add_loss, add_optimizer, evaluation):
 *   WN_COMPUTE_BF16  bf16 MFMA operands, fp32 accumulation (BASELINE configs[1]'s training dtype; the tuned path);
 *   WN_COMPUTE_F32   the reference's own arithmetic -- fp32 activations, fp32 weights, fp32 accumulation (modules.py:306-320,
 *                    wavenet.py:650-721) -- for wn_train_fwd AND wn_train_bwd (fp32 MFMA SGEMMs, ~13x slower: an accuracy /
 *                    validation mode; gradient buckets collapse to one), and for wn_synthesize: fp32 weights read from the flat
 *                    parameter buffer, fp32 ring queues, fp32 accumulation, precise tanh / exp (modules.py:273-303,
 *                    wavenet.py:821-886; launch-per-layer path only, far from real time; wn_synth_last_path() = 3). */
enum wn_compute_dtype { WN_COMPUTE_BF16 = 0, WN_COMPUTE_F32 = 1 };

#define WN_MAX_UPSAMPLE 8

/* Model + optimiser hyper-parameters: the hparams.py keys read by wavenet.py:89-208 / :522-629. */
typedef struct wn_config {
    int32_t abi_version;            /* = WN_ABI_VERSION */
    /* architecture (hparams.py:187-211) */
    int32_t layers, stacks;
    int32_t residual_channels, gate_channels, skip_out_channels, out_channels;
    int32_t kernel_size;            /* must be 3 */
    int32_t cin_channels;           /* == num_mels, multiple of 16 */
    int32_t input_type;             /* wn_input_type */
    int32_t quantize_channels;
    int32_t use_bias;
    int32_t legacy, residual_legacy;
    float   log_scale_min, log_scale_min_gauss;
    int32_t cdf_loss;
    /* upsample net (hparams.py:219-225) */
    int32_t upsample_type;          /* wn_upsample_type */
    int32_t upsample_activation;    /* wn_activation */
    int32_t n_upsample;
    int32_t upsample_scales[WN_MAX_UPSAMPLE];
    int32_t freq_axis_kernel_size;
    float   leaky_alpha;
    /* training (hparams.py:309-327) */
    float   dropout;                /* wavenet_dropout */
    int32_t clip_gradients;
    float   gradient_max_norm, gradient_max_value;
    float   adam_beta1, adam_beta2, adam_epsilon, ema_decay;
    /* capacity: workspace is sized once for these (288 GB HBM: be generous) */
    int32_t max_batch;              /* utterances per call                       */
    int32_t max_time;               /* samples per utterance (train or synth)    */
    /* global conditioning (hparams.py:228-230; wavenet.py:152-158, 669-678; modules.py:10-21, 426-432, 499-508) */
    int32_t gin_channels;           /* <= 0 disables                                                          */
    int32_t use_speaker_embedding;  /* 1: g = speaker ids looked up in the [n_speakers, gin_channels] table    */
    int32_t n_speakers;
    /* Salimans & Kingma weight normalisation of every convolution (hparams.py:323; modules.py:44-177): the exported tensors
     * become kernel (= v), g [last kernel axis], bias; kernels are used as g * v / ||v|| (norm over all axes but the last). */
    int32_t weight_normalization;
    /* 1: synthesis-only context.  Skips the saved-activation / backward workspace of training (~45 KB per (batch x time) row at the
     * paper shape; what remains -- conditioning, ring queues, mailboxes, the noise buffer -- is ~1.5 KB per row) and PRE-SIZES every
     * synthesis buffer for (max_batch, max_time), so wn_synthesize never allocates.  wn_train_* / wn_optim_step return WN_E_STATE.
     * A training context (0) can still synthesise (eval steps); it allocates its synthesis state on the first wn_synthesize. */
    int32_t inference_only;
    /* Data-parallel training: number of pieces in which wn_train_bwd completes the layer stack's gradients (wn_bwd_*bucket*), so that
     * the caller can all-reduce one piece while the next is computed.  <= 1 (single GPU): everything is final when the call ends and
     * the weight gradients run after the backward chain (measured 1.5 % faster than overlapping them when there is nothing to hide). */
    int32_t grad_buckets;
    int32_t compute_dtype;          /* enum wn_compute_dtype; hparams key mi355_compute_dtype: 'bf16' | 'fp32' */
} wn_config;

typedef struct wn_ctx wn_ctx;

/* ---- lifetime ------------------------------------------------------------------------------- */
int  wn_create(const wn_config* cfg, wn_ctx** out);     /* validates cfg (wavenet.py:94,97; models/__init__.py:6-9) */
void wn_destroy(wn_ctx* ctx);
const char* wn_last_error(const wn_ctx* ctx);           /* ctx may be NULL: error of the last failed wn_create */
int  wn_receptive_field(const wn_ctx* ctx);             /* wavenet.py:54-71; like every accessor below: WN_E_ARG for a NULL ctx */

/* ---- parameter table (host-side; replaces tf.trainable_variables(), wavenet.py:467) ---------- */
int64_t wn_param_count(const wn_ctx* ctx);              /* floats in the flat parameter buffer (incl. alignment pad) */
int     wn_num_tensors(const wn_ctx* ctx);
/* name: >=128 chars; shape: >=4 ints (TF layout) */
int     wn_tensor_info(const wn_ctx* ctx, int index, char* name, int32_t* shape, int32_t* ndim, int64_t* offset);

/* Re-pack the flat fp32 parameters into the bf16 MFMA-fragment-ordered copies the kernels read
 * (ctx-owned).  Call after every change of the parameters (i.e. after wn_optim_step). */
int wn_pack_weights(wn_ctx* ctx, const float* params, void* stream);

/* Global conditioning of the NEXT forward / synthesis call (wavenet.py:669-678 / :766-777): g = int32 speaker ids [B]
 * when cfg.use_speaker_embedding, else float [B, gin_channels].  Copied into the context (pointer borrowed for the call).
 * Required before wn_train_fwd / wn_synthesize when cfg.gin_channels > 0 ("g" must match the batch size). */
int wn_set_global_condition(wn_ctx* ctx, const void* g, int32_t B, void* stream);

/* ---- training: replaces WaveNet.step + add_loss (wavenet.py:650-721, 476-495) ----------------- */
/* x        scalar input: float [B,1,T]; mulaw-quantize: int32 class ids [B,T] (== the reference's one-hot
 *          [B,256,T], feeder.py:295-306, without materialising it)
 * c        float [B, cin, Tc], Tc*hop == T   (local conditioning, feeder.py:319-340)
 * y        targets: float [B,T,1] (scalar) or int32 [B,T] (mulaw-quantize)   (wavenet.py:488-495)
 * lengths  int32 [B]
 * dropout_seed  counter-based mask key for this step (tf.layers.dropout, modules.py:484); the same
 *          mask is regenerated in wn_train_bwd.  Dropout is disabled when cfg.dropout == 0.
 * loss_out float [1] device: masked mean loss of this batch (modules.py:798/817/836)
 * y_hat_out optional float [B, out_channels, T] (NULL to skip)                                    */
int wn_train_fwd(wn_ctx* ctx, const void* x, const float* c, const void* y, const int32_t* lengths,
                 int32_t B, int32_t T, int32_t Tc, uint64_t dropout_seed,
                 float* loss_out, float* y_hat_out, void* stream);

/* Backward of the last wn_train_fwd: writes d(loss)/d(param) for every tensor into the flat fp32
 * buffer `grads` (same layout as params; overwritten, not accumulated).
 * Replaces optimizer.compute_gradients (wavenet.py:557). */
int wn_train_bwd(wn_ctx* ctx, float* grads, void* stream);

/* Gradient buckets for data-parallel training (replaces the tower-gradient loop of wavenet.py:553-581, which averages variable by
 * variable after ALL gradients exist).  wn_train_bwd completes the flat gradient buffer in wn_bwd_num_buckets() contiguous
 * pieces, top layers first: the weight gradients of a bucket are computed on a ctx-owned low-priority stream while the serial
 * d z / d h chain is still working on the layers below.  wn_bwd_wait_bucket makes `stream` (e.g. the communication stream of the
 * caller's all-reduce) wait until bucket i of the LAST enqueued wn_train_bwd is final; the caller's own stream is ordered after
 * the whole buffer when wn_train_bwd returns, as before.  Ranges are floats into the flat buffer; the buckets are disjoint and
 * cover every tensor.  Models with weight normalisation or global conditioning report one bucket. */
int wn_bwd_num_buckets(const wn_ctx* ctx);
int wn_bwd_bucket_range(const wn_ctx* ctx, int32_t i, int64_t* offset, int64_t* count);
int wn_bwd_wait_bucket(wn_ctx* ctx, int32_t i, void* stream);

/* Stand-alone masked loss on [B,O,T] network outputs.  shift = 1: training alignment (prediction t vs sample
 * t+1, wavenet.py:488-495); shift = 0: evaluation of the incremental loop's raw outputs (wavenet.py:497-506).
 * Invalidates the saved backward state of the last wn_train_fwd. */
int wn_loss(wn_ctx* ctx, const float* y_hat, const void* y, const int32_t* lengths, int32_t B, int32_t T,
            int32_t shift, float* loss_out, void* stream);

/* ---- validation: held-out likelihood per utterance and per sample ------------------------------ */
/* Teacher-forced forward WITHOUT dropout on a training context of any cfg.dropout (evaluation: wavenet.py:342-405 computes the same
 * quantity with the incremental loop), scored per utterance.  x, c, y, lengths, B, T, Tc as wn_train_fwd.  stats_out float [B,3],
 * nll_out optional float [B,T], y_hat_out optional float [B,O,T].
 * stats_out[b] = { sum of the negative log-likelihood (nats) over the counted positions, number of counted positions, number of counted
 * positions whose loss is non-zero (the softmax head's denominator, modules.py:798) }; a position t is counted when t + 1 < min(lengths[b], T)
 * (the prediction at t is scored against sample t + 1); nll_out[b][t] is its loss, 0 where it is not counted.  An utterance without a counted
 * position gives {0, 0, 0}.  The reduction has a fixed order and uses no atomics: row b depends on row b of the inputs alone and repeats bit
 * for bit.  The launches are those of a cfg.dropout == 0 context, so y_hat equals that context's wn_train_fwd output bit for bit.
 * Arguments are validated as by wn_train_fwd; WN_E_STATE on inference-only contexts; needs wn_set_global_condition when gin_channels > 0;
 * both compute_dtype values; asynchronous on `stream`; never allocates (WN_COMPUTE_F32: its first forward reserves the fp32 state, as
 * wn_train_fwd's does); does not disturb an open stream or slot session.  Nothing is saved for a backward: wn_train_bwd returns WN_E_STATE
 * until the next wn_train_fwd.  wn_get_upsampled_features afterwards returns this batch's features. */
int wn_eval_fwd(wn_ctx* ctx, const void* x, const float* c, const void* y, const int32_t* lengths, int32_t B, int32_t T, int32_t Tc,
                float* stats_out, float* nll_out, float* y_hat_out, void* stream);
/* Stand-alone scoring of [B,O,T] network outputs (shift as wn_loss).  Writes no gradient: allowed on inference-only contexts, and it
 * does NOT invalidate the saved backward state.  B <= max_batch, T <= max_time (WN_E_SHAPE).  stats_out / nll_out as wn_eval_fwd with
 * the counted positions t + shift < min(lengths[b], T).  Calls on one context share its partial-sum scratch: one stream at a time. */
int wn_score(wn_ctx* ctx, const float* y_hat, const void* y, const int32_t* lengths, int32_t B, int32_t T, int32_t shift,
             float* stats_out, float* nll_out, void* stream);

/* Optional access to activations of the last forward (wavenet.py:702 upsampled_local_features):
 * float [B, cin, T]. */
int wn_get_upsampled_features(wn_ctx* ctx, float* out, void* stream);

/* Per-tensor clip_by_norm -> clip_by_value -> TF-Adam -> EMA, in place (wavenet.py:586-613).
 * `step` is the 0-based global step before this update; lr is the already-scheduled rate. */
int wn_optim_step(wn_ctx* ctx, float* params, const float* grads, float* adam_m, float* adam_v,
                  float* ema, float lr, int64_t step, void* stream);
/* wavenet.py:615-629 (host helper). */
float wn_learning_rate(int32_t schedule, float init_lr, int64_t step, float decay_rate,
                       int64_t decay_steps, float warmup_steps);

/* ---- synthesis: replaces WaveNet.incremental (wavenet.py:724-911) ----------------------------- */
/* Fast-WaveNet generation of T = Tc*hop samples for B streams with ring-buffer queues.
 * c           float [B, cin, Tc]  (already transposed as wavenet.py:427)
 * noise       float [T, B, noise_per_step]: MoL: M uniforms u1 then 1 uniform u2 (mixture.py:91,104);
 *             Gaussian: 1 standard-normal draw (gaussian.py:50); softmax: Q uniforms (Gumbel-max form of
 *             tf.multinomial, wavenet.py:865).  NULL => drawn on the device: Philox4x32-10 keyed by `seed`, counter = the element
 *             index of this [T, B, noise_per_step] layout (24-bit uniforms clamped to [1e-5, 1 - 1e-5], mixture.py:91,104; Gaussian draws by
 *             Box-Muller) into a ctx-owned buffer -- replaces tf.random_uniform / Normal.sample / tf.multinomial's own generator;
 *             wn_fill_noise exposes the same stream so that a run can be reproduced with an explicit buffer.
 * test_inputs optional teacher forcing (wavenet.py:877-878): float [B,T] (scalar) / int32 [B,T] ids.
 * out_samples float [B,T] (scalar types) or int32 [B,T] (class ids)   (wavenet.py:874, 897-911)
 * out_raw     optional float [B, out_channels, T] raw network outputs  (wavenet.py:847, 904-908)     */
int wn_synthesize(wn_ctx* ctx, const float* c, int32_t B, int32_t Tc, const float* noise,
                  uint64_t seed, const void* test_inputs, void* out_samples, float* out_raw,
                  int32_t steps_per_graph, void* stream);
int wn_noise_per_step(const wn_ctx* ctx);
/* The device noise stream of wn_synthesize(noise = NULL, seed): fills float [T, B, noise_per_step]. */
int wn_fill_noise(wn_ctx* ctx, float* noise, int32_t B, int32_t T, uint64_t seed, void* stream);
/* ---- wide synthesis: more than 32 utterances in one launch-per-layer run -----------------------------------------------------------
 * wn_synthesize for any 0 < B <= cfg.max_batch, for offline work (vocoding an evaluation set, GTA outputs, a data set) where samples per
 * second count and latency does not.  Always the launch-per-layer path (wn_synth_last_path() = 1): streams are the N dimension of 32-wide MFMA
 * tiles, a launch has ceil(B / 32) tiles of workgroups, and a step stays 2 L + 3 dependent launches whatever B is.  The arithmetic of a stream
 * is that of wn_synthesize(steps_per_graph > 0): its bits depend neither on its tile nor on B, and B = 1 ... 32 IS that run, bit for bit.
 * Same contract as wn_synthesize (layouts, noise == NULL => wn_fill_noise(B, T, seed) of the full B, the context's temperature pair, global
 * conditioning from wn_set_global_condition(B), test_inputs, it ends an open stream / slot session, wn_get_upsampled_features returns
 * [B, cin, T] afterwards) except:
 *   - 0 < B <= max_batch and B * T <= max_batch * max_time, else WN_E_SHAPE;
 *   - steps_per_graph <= 0 means 32 (there is no pipeline to select);
 *   - WN_E_UNSUPPORTED on compute_dtype = WN_COMPUTE_F32; WN_E_STATE before wn_pack_weights.
 * wn_synthesize, streams, the slot sessions of wn_synth_slots_begin and folded runs keep their limit of 32 streams (wide slot sessions:
 * wn_synth_wide_slots_begin below).
 * State: its own queues, per-step scratch and captured graph (a wide run never evicts the graph of the <= 32 path), sized for
 * 32 * ceil(B / 32) streams.  A training context grows it to the largest B seen; an inference-only context (which may now have
 * max_batch > 32: the pipeline, the streaming state and the slot tables are then sized for 32, the wide state for max_batch, and only when
 * max_batch > 32) sizes it at wn_create and wn_synthesize_wide never allocates there.
 * Memory (computed from the layouts, not measured): the queues hold sum_l 4 d_l rows of R bf16 per stream -- the paper model (24 layers in 2
 * stacks, d <= 2 048, R = 256): 32 760 rows x 256 x 2 B = 16.8 MB per stream, 17 GB at 1 024 streams; the upsampled conditioning is about 0.5 KB per
 * stream-sample (cin bf16 rows + the fp32 levels of the upsample net): 54 GB for 1 024 streams x 5 s at 22 050 Hz.  The run that bounds
 * the latter is the wide slot session (wn_synth_wide_slots_begin): its conditioning is upsampled push by push. */
int wn_synthesize_wide(wn_ctx* ctx, const float* c, int32_t B, int32_t Tc, const float* noise,
                       uint64_t seed, const void* test_inputs, void* out_samples, float* out_raw,
                       int32_t steps_per_graph, void* stream);
/* ---- sampling temperature: tempered noise for every head, path and slot ---------------------------------------------------------
 * All samplers consume noise in a form where temperature is a change of the NOISE ENTRY, not of the sampler:
 *   select   (Gumbel-max choice of a mixture component / a class)  argmax(logit_i - log(-log u_i))     u' = exp(-(-ln u)^tau)        (the Gumbel term x tau)
 *   logistic (MoL: the draw of the chosen component)               mu + exp(ls) (log u - log(1 - u))   u' = 1 / (1 + exp(-tau logit u))  (the logit x tau)
 *   normal   (Gaussian head)                                       mu + exp(ls) eps                    eps' = tau eps
 * with u' clamped to the samplers' range [1e-5, 1 - 1e-5].  tau_scale applies to the logistic / normal draw, tau_select to the select entries
 * (MoL: the first M of a sample's M + 1 entries; softmax: all Q; the Gaussian head has none).  Valid: finite, 0 <= tau <= 2, else WN_E_ARG.
 * tau == 1 returns the entry untouched (bit-identical to the untempered run); tau == 0 is the deterministic decode: the arg-max component's
 * mean clipped to [-1, 1] / the arg-max class (entries become the constants exp(-1), 0.5, 0).  For tau <= 1 the clamp never acts; for tau > 1 it
 * TRUNCATES the tails (an entry that would leave the range is pulled back to its end), so the tails are lighter than tau asks for.
 * The context's pair (default (1, 1) at wn_create) is HOST state read by wn_synthesize and by every wn_synth_stream_push at the time of the call:
 * setting it ends no stream or session, and wn_pack_weights does not reset it.  Device noise (noise == NULL) is generated already tempered;
 * caller noise with a pair other than (1, 1) is tempered into the context's noise buffer (reserved exactly as for device noise: an
 * inference-only context keeps its pre-sized buffer and its WN_E_SHAPE) and the run reads that copy -- the caller's buffer is not written; with
 * (1, 1) the caller's pointer is passed through as before.  wn_fill_noise stays UNTEMPERED: bit for bit,
 *   wn_synthesize(noise = NULL, seed) at tau  ==  wn_synthesize(noise = wn_temper_noise(wn_fill_noise(seed), tau)) at (1, 1).
 * No sampling kernel changes and the per-sample time is unchanged: the work is fused into the noise kernels that run once before a span. */
int wn_synth_set_temperature(wn_ctx* ctx, float tau_scale, float tau_select);
int wn_synth_get_temperature(const wn_ctx* ctx, float* tau_scale, float* tau_select);
/* Temper a noise buffer: in / out device float [T, B, noise_per_step] of this context's head, in == out allowed; asynchronous on `stream`.
 * Also the way to give wn_sample (the train-time log path) a temperature: temper the noise it is passed. */
int wn_temper_noise(wn_ctx* ctx, const float* in, float* out, int32_t B, int32_t T, float tau_scale, float tau_select, void* stream);
/* wn_synthesize enqueues and returns (no device synchronisation).  The persistent pipeline bounds every hand-off spin; if one times
 * out (a workgroup was not resident) the kernels leave early and raise a device flag.  wn_synth_check waits for the LAST
 * wn_synthesize of this context to finish and returns WN_E_HIP (+ wn_last_error) if that happened, WN_OK otherwise; the next
 * wn_synthesize on the context reports a pending failure too.  wn_synth_last_path: 0 none yet, 1 launch-per-layer hipGraph path,
 * 2 persistent pipeline, 3 fp32 launch-per-layer path (compute_dtype = WN_COMPUTE_F32). */
int wn_synth_check(wn_ctx* ctx);
int wn_synth_last_path(const wn_ctx* ctx);
/* 1 if wn_synthesize(steps_per_graph <= 0) would run B streams of this model on the persistent pipeline (all of a CU's weights must
 * fit its 160 KiB of LDS next to 256 B of state per stream: one CU per 32 gate pairs, <= 8 CUs per layer, R, S <= 384, B <= 32), 0 if
 * it would take the launch-per-layer hipGraph path.  Host helper: a caller sends the whole batch in one run when this says 1 for it.
 * Per generated sample on the paper model (R = S = 256, 24 layers; deadline 45.35 us at 22.05 kHz): 28 us for 1 ... 12 streams, ~1.7 us per
 * stream beyond -- 16: 36 us, 20: 42.5 us (real time), 24: 49 us; a model whose CUs fit the chip more than once is cut into several runs side by
 * side in the same launch (wn_synth_last_instances: hparams.py's default model serves 20 streams at 26 us per sample). */
int wn_synth_pipe_eligible(const wn_ctx* ctx, int32_t B);
/* 16-bit storage type of the persistent pipeline's weights, hand-off granules and ring queues for the NEXT runs of this context
 * (fp32 accumulation either way): 1 = IEEE half (the default: raw outputs 1.2e-3 from the reference's fp32 loop at C4's model, 34.8 us per
 * sample), 0 = bf16 (8.7e-3, 35.0 us; 8 exponent bits).  A half run whose residual stream leaves the half range (|x| > 65504) is
 * reported by wn_synth_check / the next wn_synthesize as WN_E_HIP ("left the half-precision range"): switch to bf16 and run again.
 * Environment at wn_create: WN_PIPE_DTYPE=fp16|bf16 (case-insensitive; also f16 / half / float16 / bfloat16; anything else fails wn_create). */
int wn_synth_pipe_dtype(wn_ctx* ctx, int32_t half);
/* How the LAST wn_synthesize of this context ran, as the library configured it (not as the environment asked): fills up to `cap` of
 * out[0] path (as wn_synth_last_path) and, for a pipeline run, out[1] instances, [2] batched pre-multiplication, [3] kernel specialisation
 * (0 generic, 1 paper widths R = S = 256, 2 hparams.py widths R = S = 128), [4] storage (1 IEEE half, 0 bf16), [5] head CUs, [6] early
 * requests from this many streams, [7] abort word tested every n streams (0: once per sample), [8] workgroups launched, [9] streams of the
 * largest instance; zeros for the other paths.  Returns the number of entries written (10) or WN_E_ARG.  bench.py records it next to
 * every timed synthesis leg. */
int wn_synth_last_config(const wn_ctx* ctx, int32_t* out, int32_t cap);
/* how many pipeline INSTANCES the last wn_synthesize ran side by side (1 for a run of <= 10 streams or a model whose CUs fit the chip once:
 * the paper model takes 193 of 256; hparams.py's default model 81: up to three instances of <= 10 streams each). */
int wn_synth_last_instances(const wn_ctx* ctx);
/* 1 if the last wn_synthesize ran the persistent pipeline with the BATCHED pre-multiplication (R = 256 models, any eligible run of <= 32 streams: the
 * past taps and conditioning of every stream's next sample are multiplied in one [64 x K] x [K x streams] matrix product per sample and CU
 * instead of one matvec per stream), 0 otherwise.  Environment: WN_PIPE_BATCHPRE=0 keeps the per-stream form (A/B switch). */
int wn_synth_last_batched(const wn_ctx* ctx);

/* ---- streaming synthesis: the same generation as ONE wn_synthesize, cut into pushes of mel frames as they arrive ------------
 * The reference's loop is a streaming computation (zero queues, wavenet.py:815-816; silence input, :433-445; step t reads only its
 * own conditioning frame and the queues, :821-886): a stream continues the ring queues, the time index, the fed-back sample and the
 * device noise counter across pushes, and the samples it returns are bit-identical to one wn_synthesize over the concatenated frames
 * (same B, seed, steps_per_graph, noise / teacher forcing).  One open stream per context, B <= 32 utterances in lockstep (independent utterances: the slot sessions below).
 *
 * Mel frames of context the upsample net needs on each side of a frame (host only: no context, no GPU): 0 / 0 for 'NearestNeighbor',
 * '2D' and '1D' (time kernel == stride); 'SubPixel': ceil(h / hop) on both sides with h = sum_i prod_{k >= i} s_k samples (layer i's 3-tap
 * time kernel reaches one of its input samples); 'Resize': ceil(h / hop) with h = sum_i p_i * prod_{k > i} s_k samples, p_i = (s_i - 1) / 2
 * on the left, s_i - 1 - p_i on the right (the s-tap SAME kernels). */
int wn_synth_stream_lookahead(const wn_config* cfg, int32_t* frames_left, int32_t* frames_right);
/* Open a stream of B utterances at t = 0.  The path is chosen as wn_synthesize(steps_per_graph) would for B and kept for the life of the
 * stream (the fp32 launch-per-layer path for compute_dtype = WN_COMPUTE_F32).  seed: the device noise of wn_synthesize(noise = NULL, seed) over the
 * whole utterance.  Global conditioning: what wn_set_global_condition set, captured here.  Ends any stream already open on the context.
 * Allocates only what a wn_synthesize of B streams would (nothing on inference-only contexts). */
int wn_synth_stream_begin(wn_ctx* ctx, int32_t B, uint64_t seed, int32_t steps_per_graph, void* stream);
/* Append Tn >= 0 frames, c = float [B, cin, Tn], and generate every frame whose conditioning is now complete: frames [done, pushed -
 * frames_right), with final = 1 [done, pushed).  That is n = frames * hop samples: out_samples [B, n] (float or int32 as wn_synthesize),
 * optional out_raw [B, O, n], optional noise [n, B, noise_per_step] (NULL: the device stream of `seed`, continued), optional
 * test_inputs [B, n].  *n_out (host) = n, known at enqueue time (no synchronisation).  n may be 0.  Asynchronous and ordered like
 * wn_synthesize; never allocates.  WN_E_SHAPE if n > max_time or B x (window frames) x hop exceeds max_batch x max_time (window =
 * frames_left of context + the frames not yet generated).  After final = 1 the stream is closed.  WN_E_STATE: no stream open, or the
 * stream was ended by wn_synthesize / wn_pack_weights / wn_set_global_condition / wn_synth_pipe_dtype, or poisoned: a pipeline run of
 * this stream that wn_synth_check (or the next push) reported failed.  wn_train_fwd / wn_train_bwd between pushes do not disturb it.
 * wn_get_upsampled_features afterwards returns the features of the span this push generated. */
int wn_synth_stream_push(wn_ctx* ctx, const float* c, int32_t Tn, int32_t final, const float* noise, const void* test_inputs,
                         void* out_samples, float* out_raw, int32_t* n_out, void* stream);
/* Abandon the open stream (no device work; what was pushed and not generated is dropped).  A later push returns WN_E_STATE. */
int wn_synth_stream_end(wn_ctx* ctx);

/* ---- synthesis slots: utterances join and leave a running batch (continuous batching for the vocoder) -----------------------
 * A session is B slots (B <= 32, B <= max_batch) served by ONE path / pipeline configuration -- the one wn_synthesize(steps_per_graph) would take
 * for B -- for the life of the session.  Every slot is idle or carries one utterance with its own t = 0, seed, global condition and mel frames;
 * utterances are opened, fed, finished and replaced independently.  A slot's out_samples / out_raw depend only on the session's B and configuration,
 * the slot index and the slot's own frames, noise, teacher forcing and condition -- not on how the frames were cut into pushes, when the slot was
 * opened, what the other slots do or what occupied it before -- and are bit-identical to ONE wn_synthesize of the same B and steps_per_graph with the
 * utterance's frames in batch row = slot index and, for device noise, column b of the [T, B, nps] noise = wn_fill_noise(B = 1, T, seed_b) tempered
 * (wn_temper_noise) by slot b's pair -- the context's pair at wn_synth_slot_open, or what wn_synth_set_slot_temperature set since, push by push; caller
 * noise is tempered column by column in the same way into the context's buffer.
 * Frames -> samples follow wn_synth_stream_lookahead per slot: a slot generates its frames [done, pushed - frames_right), all of them with final.
 * A push runs max_b n_out[b] steps; slots with nothing (more) to generate take part as dummy steps that write nothing (no queue row, no output
 * element, no abort).  Reopening a slot clears nothing: a tap before the utterance's own t = 0 is invalid per slot.
 * Errors: WN_E_STATE for a call without a session, open of a live slot, frames for an idle slot, a session ended by wn_synthesize / wn_pack_weights /
 * wn_synth_pipe_dtype / wn_synth_stream_begin, or poisoned by a failed pipeline run (reported by wn_synth_check or the next push); WN_E_SHAPE when a
 * push would generate more than max_time samples for a slot or a slot's window exceeds the workspace (a rejected push leaves every slot as it was);
 * WN_E_UNSUPPORTED from wn_synth_slots_begin on compute_dtype = WN_COMPUTE_F32 (the fp32 validation mode has no slot sessions).  A session and a
 * stream exclude one another on a context; wn_train_fwd / wn_train_bwd between pushes do not disturb a session; wn_set_global_condition is not
 * used (the condition is per slot).  Inference-only contexts never allocate in these calls. */
int wn_synth_slots_begin(wn_ctx* ctx, int32_t B, int32_t steps_per_graph, void* stream);
/* The slot becomes live at its own t = 0 with the next push.  g: this utterance's global condition on the device -- one int32 speaker id
 * (use_speaker_embedding) or float [gin_channels]; NULL iff gin_channels <= 0.  seed: the slot's device noise (noise = NULL pushes). */
int wn_synth_slot_open(wn_ctx* ctx, int32_t slot, uint64_t seed, const void* g, void* stream);
/* Override the sampling temperature of a LIVE slot (wn_synth_slot_open copied the context's pair into it), from the next push on (host only).
 * WN_E_STATE without a session or for an idle slot; WN_E_ARG for a slot outside the session or a temperature outside [0, 2]. */
int wn_synth_set_slot_temperature(wn_ctx* ctx, int32_t slot, float tau_scale, float tau_select);
/* c float [B, cin, Tn] (rows of idle slots ignored); frames[b] in [0, Tn] (host): the leading frames of row b appended to slot b; final_[b] != 0
 * (host): slot b's utterance ends with these frames and the slot is idle afterwards.  n_out[b] (host) = samples generated for slot b, known at
 * enqueue time.  out_samples [B, out_pitch] (float / int32 as wn_synthesize), optional out_raw [B, O, out_pitch], optional test_inputs
 * [B, out_pitch], out_pitch >= max_b n_out[b]; elements beyond n_out[b] of a row keep the caller's bytes.  noise [max_b n_out[b], B, nps] indexed by
 * the push-local step (rows of slots that do not generate are ignored) or NULL.  Asynchronous, ordered like wn_synthesize, never synchronises.
 * wn_get_upsampled_features afterwards returns [B, cin, max_b n_out[b]]: row b = the conditioning slot b's n_out[b] steps read. */
int wn_synth_slots_push(wn_ctx* ctx, const float* c, int32_t Tn, const int32_t* frames, const int32_t* final_, const float* noise,
                        const void* test_inputs, void* out_samples, float* out_raw, int32_t out_pitch, int32_t* n_out, void* stream);
int wn_synth_slot_abandon(wn_ctx* ctx, int32_t slot);              /* drop a live utterance (host only, no device work); the slot is idle */
int wn_synth_slot_frames_done(const wn_ctx* ctx, int32_t slot);    /* frames generated so far, -1 idle; WN_E_ARG / WN_E_STATE */
int wn_synth_slots_end(wn_ctx* ctx);
/* ---- wide slot sessions: more than 32 slots on the launch-per-layer path -------------------------------------------------------
 * The same kind of session for any 0 < B <= max_batch: continuous batching at the width of wn_synthesize_wide.  Always the launch-per-layer path
 * (wn_synth_last_path() = 1) on the wide owner -- the queues, runner and captured graph of wn_synthesize_wide, ceil(B / 32) tiles of 32 slots per
 * launch; steps_per_graph <= 0 means 32.  Every other call of the session is shared, with host arrays of B entries: wn_synth_slot_open,
 * wn_synth_set_slot_temperature, wn_synth_slots_push, wn_synth_slot_abandon, wn_synth_slot_frames_done, wn_synth_slots_end.
 * Contract: that of the slot sessions above, restated for width.  A slot's out_samples / out_raw depend only on the slot's own frames, noise,
 * teacher forcing, condition and temperature pair -- not on B, the slot's tile, how the frames were cut into pushes, when the slot was opened, what the
 * other slots (or whole other tiles) do or what occupied it before.  They are bit-identical to wn_synthesize(steps_per_graph > 0) of <= 32 streams with
 * the utterance in row slot & 31, and to wn_synthesize_wide with the utterance in row slot; for device noise the column is
 * wn_fill_noise(B = 1, T, seed_slot) tempered by the slot's pair.  A tile without a live slot runs as dummy steps that store nothing.
 * Errors: as above, and WN_E_SHAPE for B outside (0, max_batch] (an inference-only context: the width its wide state was sized for),
 * WN_E_UNSUPPORTED on WN_COMPUTE_F32, WN_E_STATE before wn_pack_weights.  One session at a time per context, narrow or wide: either begin ends the
 * other's, as wn_synthesize, wn_synthesize_wide, wn_pack_weights, wn_synth_pipe_dtype and wn_synth_stream_begin do.  A rejected push leaves every slot
 * as it was.  The session tables are sized for the session's B: a training context grows them at begin; an inference-only context with
 * max_batch > 32 sizes them for max_batch at wn_create and never allocates in these calls.  A push never synchronises.
 * Memory (computed from the layouts, not measured): the queues are those of wn_synthesize_wide (16.8 MB per slot on the paper model).  The
 * conditioning is upsampled per push: the tables of the push (cin bf16 rows + fp32 rows) and the upsample workspace hold at most max_batch x max_time
 * stream-samples (about 0.5 KB each), where max_time need only cover ONE push (a slot generates at most max_time samples per push), not the
 * utterance: 1 024 slots x 8 frames of 256 samples = 2.1 M stream-samples, about 1 GB, whatever the utterances' lengths.  The pending mel windows are
 * 2 x B x cin x capw floats, capw = max_time / hop + lookahead + 1 frames per slot. */
int wn_synth_wide_slots_begin(wn_ctx* ctx, int32_t B, int32_t steps_per_graph, void* stream);

/* ---- folded synthesis: ONE utterance generated as overlapping segments that run side by side (WaveRNN's fold_with_overlap / xfade_and_unfold) ----
 * Streams and slots spend the width of a run on more utterances; a folded run spends it on one.  The utterances are cut into rows; row r generates
 * the mel frames [first, first + frames) of utterance `utt` from a cold start (silence, zero queues, its own t = 0) as one row of ONE slot-form span.
 * Its samples before frame `keep` are warm-up and are discarded; over the frames [keep, keep + fade) it fades in against the fade-out of the previous
 * row of the same utterance; from keep + fade on it is the output until the next row's fade begins.  A row is NOT the continuation of its predecessor:
 * the waveform differs from the one-shot run's after the first seam (how audible a seam is depends on the model; nothing here smooths beyond the fade).
 * Rules a plan obeys (wn_fold_check; wn_fold_plan's output does): rows are sorted by utterance, every utterance 0 ... U - 1 has at least one;
 * 0 <= first <= keep, fade >= 0, keep + fade <= first + frames <= the utterance's frames, frames >= 1; the first row of an utterance has first = keep =
 * fade = 0, its last row ends at the utterance's last frame; consecutive rows r, r + 1 of an utterance: keep[r+1] + fade[r+1] == first[r] + frames[r]
 * and keep[r+1] >= keep[r] + fade[r]. */
typedef struct wn_fold_row { int32_t utt, first, frames, keep, fade; } wn_fold_row;   /* all in mel frames of utterance `utt` */
/* Planner (host only: no context, no GPU; deterministic).  Every utterance gets one row; the remaining rows, up to rows_max <= 32, go one at a time to
 * the utterance whose rows are currently longest (frames / rows; ties: the lowest index), until another row would leave it fewer than min_keep new
 * frames per row -- an utterance shorter than 2 * min_keep stays one row, so a folded run of it is the one-shot run.  An utterance of F frames in k rows
 * has the boundaries a_j = floor(j F / k); row j has keep = a_j, first = max(0, a_j - warm), fade = min(fade, a_{j+1} - a_j) for j > 0 and ends at
 * a_{j+1} + fade of row j + 1 (F for the last).  Returns the number of rows written to rows[0 .. cap), WN_E_ARG (null pointer, U < 1, a length < 1,
 * warm / fade < 0, min_keep < 1) or WN_E_SHAPE (rows_max outside [U, 32], cap too small). */
int wn_fold_plan(const int32_t* utt_frames, int32_t U, int32_t rows_max, int32_t warm, int32_t fade, int32_t min_keep, wn_fold_row* rows, int32_t cap);
/* The rules above on a caller's plan (host only).  WN_OK, or WN_E_ARG with a message naming the row in msg[0 .. cap) (msg may be NULL). */
int wn_fold_check(const int32_t* utt_frames, int32_t U, const wn_fold_row* rows, int32_t n_rows, char* msg, int32_t cap);
/* One call, asynchronous on `stream`, never synchronises.  c float [U, cin, F_max], F_max = max_u utt_frames[u] (utterance u: its leading utt_frames[u] frames), utt_frames
 * and rows HOST arrays (free when the call returns), rows validated by wn_fold_check (WN_E_ARG naming the row).  With n_max = max_r frames[r] * hop it enqueues
 *   (a) the upsample net ONCE over the whole utterances (utterances of equal length as one batch): a row reads exactly the conditioning rows the one-shot
 *       run reads, whatever the lookahead of 'SubPixel' / 'Resize';
 *   (b) the fold: rows [first * hop, (first + frames) * hop) of each row's utterance into the session table [n_rows][n_max][cin] (and test_inputs likewise);
 *   (c) the gate-bias row of each row's utterance; g: device, U int32 speaker ids (use_speaker_embedding) or float [U, gin_channels]; NULL iff gin_channels <= 0;
 *   (d) noise [n_max, n_rows, noise_per_step] or NULL: column r = the one-stream device noise of seed + r (wn_fill_noise(B = 1, seed + r)); either is
 *       tempered by the context's pair;
 *   (e) ONE span in the slot form (every row from its own t = 0, frames[r] * hop samples, dummy steps behind) on the path wn_synthesize(steps_per_graph) would
 *       take for n_rows streams: row r is bit-identical to row r of ONE wn_synthesize(B = n_rows) whose row r holds these conditioning rows;
 *   (f) the unfold: out_wav float [U, wav_pitch], wav_pitch >= max_u utt_frames[u] * hop: the DECODED waveform in [-1, 1] (wn_inv_mulaw / wn_inv_mulaw_quantize
 *       of the model-domain samples; identity for 'raw'), fl(fl(a * w_out[i]) + fl(b * w_in[i])) inside a fade of n = fade * hop samples (a: the previous row,
 *       b: this one) and the row's decoded sample elsewhere; elements beyond an utterance's length keep the caller's bytes.  fade_kind 0, equal power:
 *       w_in[i] = sin(pi / 2 * (i + 0.5) / n), w_out[i] = cos(pi / 2 * (i + 0.5) / n); 1, linear: w_in[i] = (i + 0.5) / n, w_out[i] = 1 - w_in[i] -- float32
 *       tables computed on the host in double.  No atomics, a fixed order: two runs agree bit for bit.
 * test_inputs optional [U, wav_pitch] teacher forcing in the MODEL domain (float / int32 ids as wn_synthesize); out_rows optional [n_rows, row_pitch] model-domain
 * samples of every row, out_raw optional float [n_rows, out_channels, row_pitch], row_pitch >= n_max when either is given (elements beyond a row's samples keep
 * the caller's bytes).  Without out_rows the rows live in context scratch of max_batch x max_time elements, as the gathered test_inputs do: n_rows x row_pitch
 * must fit it then.
 * WN_E_SHAPE: n_rows > min(32, max_batch), n_max > max_time, n_rows x n_max or a group's utterances x frames x hop beyond max_batch x max_time.  WN_E_UNSUPPORTED on
 * compute_dtype = WN_COMPUTE_F32 (as slot sessions); WN_E_STATE before wn_pack_weights.  Ends an open stream or slot session, as wn_synthesize does; a failed pipeline
 * run is reported by wn_synth_check / the next call and poisons nothing opened afterwards.  Allocates what a slot session of n_rows would (nothing on inference-only
 * contexts: the row scratch is reserved with the slot tables).  wn_get_upsampled_features afterwards returns [n_rows, cin, n_max], as after a slot push.
 * wn_set_global_condition is not used. */
int wn_synthesize_folded(wn_ctx* ctx, const float* c /*[U, cin, F_max]*/, const int32_t* utt_frames /*host [U]*/, int32_t U,
                         const wn_fold_row* rows /*host*/, int32_t n_rows, int32_t fade_kind /*0 equal power, 1 linear*/,
                         const void* g, const float* noise, uint64_t seed, const void* test_inputs,
                         float* out_wav /*[U, wav_pitch]*/, int32_t wav_pitch,
                         void* out_rows /*optional [n_rows, row_pitch]*/, float* out_raw /*optional [n_rows, O, row_pitch]*/,
                         int32_t row_pitch, int32_t steps_per_graph, void* stream);
/* test hook of the tables above (host only): w_in / w_out float [n]; WN_E_ARG for n < 1, a kind outside 0 ... 1 or a null pointer */
int wn_fold_weights(int32_t fade_kind, int32_t n, float* w_in, float* w_out);

/* Stand-alone samplers on [B,O,T] parameters (train-time log path, wavenet.py:302-325).  Temperature: wn_temper_noise on `noise` first. */
int wn_sample(wn_ctx* ctx, const float* y_hat, int32_t B, int32_t T, const float* noise /*[T,B,nps]*/,
              void* out /* float [B,T] or int32 [B,T] */, void* stream);

/* ---- mu-law codec (wavenet_vocoder/util.py:30-129; mu fixed to 255 as the reference does) ------ */
int wn_mulaw(const float* x, float* y, int64_t n, void* stream);
int wn_inv_mulaw(const float* y, float* x, int64_t n, void* stream);
int wn_mulaw_quantize(const float* x, int32_t* q, int64_t n, void* stream);        /* bit-exact vs numpy */
int wn_inv_mulaw_quantize(const int32_t* q, float* x, int64_t n, void* stream);
/* argmax over channels of [B,Q,T] logits -> int32 [B,T] (first max wins, like tf.argmax) */
int wn_argmax_channels(const float* logits, int32_t* out, int32_t B, int32_t Q, int32_t T, void* stream);

/* ---- mel analysis: wav -> mel-spectrogram (the reference's preprocessing front end: librosa.stft + librosa.filters.mel + numpy) ----
 * A context of its own, independent of wn_ctx: no model is needed.  For an utterance of n samples the analysis gives F = 1 + n / hop_size
 * frames (librosa.stft, center = True, pad_mode = 'constant'): frame f is the win_size samples around f * hop_size under a periodic Hann
 * window centred in n_fft, its DFT bins 0 ... n_fft / 2, |.|^magnitude_power, the mel filters, 20 log10(max(10^(min_level_db / 20), .)) -
 * ref_level_db, and -- signal_normalization -- one of the four _normalize variants (allow_clipping x symmetric_mels), without the assert of
 * the two that do not clip.  Exact fp32 products (the fp32 matrix instruction) with fp32 accumulation in a fixed order: two runs, and an
 * utterance alone or inside any batch, are bit-identical.  Optionally fused into the read of the signal:
 *   y[s] = gain[b] * (x[s] - preemphasis * x[s - 1]),  x[-1] = 0   (audio.py:22-25 and the rescale of wavenet_preprocessor.py:76);
 * preemphasis = 0 and gain = NULL analyse x itself.  Status codes, wn_mel_last_error and the stream convention are those of the header's top.
 * Device memory -- the [win_size, 2 x (1 + n_fft / 2)] DFT basis (10 MB at the default geometry, padded to whole bin groups) and the mel filters -- is reserved in
 * wn_mel_create; wn_mel_run and wn_mel_peak never allocate, and lengths travel as kernel arguments (the host array is free when the call
 * returns).  max_batch = 0 makes a geometry-only context: nothing is reserved, no device is touched, wn_mel_num_frames works and wn_mel_run /
 * wn_mel_peak refuse every B.  Limits: num_mels <= 128, n_fft <= 65536, and the signal span of 32 frames, 31 hop_size + win_size floats,
 * must fit the 160 KiB LDS (WN_E_UNSUPPORTED otherwise). */
typedef struct wn_mel_config {
    int32_t abi_version;            /* = WN_ABI_VERSION */
    int32_t sample_rate;            /* informational (the caller built mel_basis for it) */
    int32_t n_fft, hop_size, win_size, num_mels;                  /* hparams.py:102-110; win_size <= n_fft, n_fft even */
    float   magnitude_power;        /* > 0; 2 and 1 take no transcendental */
    float   min_level_db, ref_level_db, max_abs_value;            /* hparams.py:126-133 */
    float   preemphasis;            /* k of y[s] = x[s] - k x[s - 1]; 0: off */
    int32_t signal_normalization, allow_clipping, symmetric_mels; /* allow_clipping = hparams allow_clipping_in_normalization */
    int32_t max_batch;              /* utterances per call; 0: geometry-only context */
    int64_t max_samples;            /* samples per utterance */
} wn_mel_config;
typedef struct wn_mel wn_mel;

/* audio.py:70-77, 178-182, 243-270.  mel_basis: HOST float [num_mels, 1 + n_fft / 2] (librosa.filters.mel; any dense matrix is honoured).
 * Validation before any device call: WN_E_SHAPE for n_fft odd, win_size > n_fft, hop_size < 1, num_mels < 1; WN_E_ARG for
 * magnitude_power <= 0, a null pointer, a foreign abi_version.  wn_mel_last_error with NULL gives the text of a failed create. */
int  wn_mel_create(const wn_mel_config* cfg, const float* mel_basis, wn_mel** out);
void wn_mel_destroy(wn_mel* mel);
const char* wn_mel_last_error(const wn_mel* mel);
/* audio.py:178-182 (librosa.stft, center = True): 1 + n_samples / hop_size; WN_E_ARG for a NULL context or n_samples < 0 (host only) */
int64_t wn_mel_num_frames(const wn_mel* mel, int64_t n_samples);
/* the largest number of frames a workgroup of this context takes (32, 64 or 128; 0: geometry-only).  wn_mel_run picks 32, 64 or 128 up to this per
 * call from the batch's frame counts; the result never depends on the pick (every frame's sums run in the same order).  Tests place utterance
 * lengths around its multiples.  Environment at wn_mel_create: WN_MEL_TF=32|64|128 pins one tile (the A/B switch of tools/mel_timing.py). */
int  wn_mel_frame_tile(const wn_mel* mel);
/* peak[b] = max_s |x[s] - preemphasis * x[s - 1]| over the utterance's lengths[b] samples (0 for an empty one): exact and order independent,
 * equal to numpy's float32 result.  With it a device-resident caller forms the gain rescaling_max / max |preem_wav| of
 * wavenet_preprocessor.py:76 (audio.py:22-25) without a host round trip.  wav: device float [B, ld]; lengths: HOST int32 [B]; peak: device float [B]. */
int  wn_mel_peak(wn_mel* mel, const float* wav, int64_t ld, const int32_t* lengths, int32_t B, float* peak, void* stream);
/* audio.py:70-77 melspectrogram of a ragged batch.  wav: device float [B, ld], row b holds lengths[b] <= ld samples (HOST int32 [B]); gain:
 * device float [B] or NULL (= 1).  out: device float [B, F_max, num_mels] (channels_first = 0: the mels/mel-*.npy layout) or [B, num_mels,
 * F_max] (1: the layout wn_synthesize takes as c); rows f >= 1 + lengths[b] / hop_size hold the value an all-zero signal gives (-max_abs_value
 * under the default hparams: the synthesiser's pad).  WN_E_SHAPE: B > max_batch, lengths[b] > ld or > max_samples, F_max < the frames of
 * the longest utterance. */
int  wn_mel_run(wn_mel* mel, const float* wav, int64_t ld, const int32_t* lengths, const float* gain, float* out, int32_t B, int32_t F_max,
                int32_t channels_first, void* stream);

/* ---- output stage: model-domain samples -> de-emphasised float32 and / or 16-bit PCM on the device -------------------------------
 * A handle of its own, independent of wn_ctx: it takes any device buffer a synthesis call produced (wn_synthesize, wn_synth_stream_push,
 * wn_synth_slots_push: in_type = the model's input type; wn_synthesize_folded's out_wav: in_type 0).  Per sample, strictly in sample order,
 *   x = decode(in)                      exactly wn_inv_mulaw (1) / wn_inv_mulaw_quantize (2), the identity for 0
 *   y[t] = fl32(fl32(k y[t-1]) + x[t])  a separately rounded multiply and add (never an fma); k = 0 does no arithmetic: y has the bits of x
 *   PCM = trunc(clamp(fl32(y s), -32767, 32767))
 * so a row is bit-identical however it is cut into pushes.  Results of magnitude below 2^-126 are unspecified (flushed or gradual).  One workgroup
 * per row walks it in blocks: all lanes decode into LDS, one lane runs the chain, all lanes convert and store; rows of a call run side by side.
 * The carried state (y[-1] per row) and a scratch for wn_post_finish's peaks are reserved in wn_post_create; no call allocates or synchronises, lengths
 * travel as kernel arguments (the host arrays are free when the call returns).  Calls on one handle belong on one stream at a time.  Elements of a row
 * beyond n[b] keep the caller's bytes in both outputs.  Validation before any device call: WN_E_ARG for a null pointer, a foreign abi_version,
 * max_rows < 1, in_type outside 0 ... 2, deemphasis outside [0, 1) or not finite, gain not finite or <= 0, B < 1, a negative n[b], no output at all
 * (push) or no out_f32 (finish); WN_E_SHAPE for B > max_rows or a pitch (in elements) smaller than the longest row. */
typedef struct wn_post_config {
    int32_t abi_version;   /* = WN_ABI_VERSION */
    int32_t max_rows;      /* rows of carried state, >= 1 */
    int32_t in_type;       /* 0: float, already a waveform ('raw', or wn_synthesize_folded's out_wav)
                              1: float mu-law domain ('mulaw')      2: int32 class ids ('mulaw-quantize') */
    float   deemphasis;    /* k of y[t] = x[t] + k y[t-1]; 0 <= k < 1; 0: off */
    float   gain;          /* wn_post_push only: PCM = y * gain * 32767; finite, > 0 */
} wn_post_config;
typedef struct wn_post wn_post;
int  wn_post_create(const wn_post_config* cfg, wn_post** out);
void wn_post_destroy(wn_post* p);
const char* wn_post_last_error(const wn_post* p);   /* NULL: text of the last failed create */
/* chunk form: continues row b's filter from where its last push left it; restart[b] != 0 (NULL: none) starts row b from y[-1] = 0.  n[b] = 0 leaves
 * row b's state alone unless it is restarted.  s = (float)(gain * 32767.0).  n, restart: HOST int32 [B]; out_f32 / out_pcm: device [B, out_pitch], either
 * may be NULL; clipped: device int32 [B] or NULL, the number of samples of THIS call with |fl32(y s)| > 32767 (written, not accumulated). */
int wn_post_push(wn_post* p, const void* in, int64_t in_pitch, const int32_t* n, const int32_t* restart, int32_t B,
                 float* out_f32, int16_t* out_pcm, int64_t out_pitch, int32_t* clipped, void* stream);
/* whole-utterance form: every row from y[-1] = 0 and peak-normalised as save_wavenet_wav does it (audio.py:17-20): peak[b] = max_t |y[b, t]| over the
 * row's n[b] samples, s = (float)(32767.0 / max(0.01, (double)peak[b])) formed on the device.  Two launches (chain + peak, then the conversion), no host
 * synchronisation.  Neither reads nor writes the carried state.  out_f32 required, out_pcm and peak (device float [B]) optional. */
int wn_post_finish(wn_post* p, const void* in, int64_t in_pitch, const int32_t* n, int32_t B,
                   float* out_f32, int16_t* out_pcm, int64_t out_pitch, float* peak, void* stream);

/* ---- reconstruction check: how far the mel-spectrogram a of a generated signal is from the conditioning b it was generated from ----
 * A handle of its own, independent of the model context, like the mel analysis and the output stage: it takes any two device mel buffers, each
 * channels-first [B, num_mels, pitch] (how the synthesis calls take c, and the analysis' channels-first output) or channels-last [B, pitch, num_mels]
 * (the mel-*.npy layout), pitch >= the longest row; row b compares its first frames[b] frames and elements at f >= frames[b] are never read into a
 * result.  All float32, every operation rounded on its own except the dot products, which are fused multiply-adds in channel order.  D is the
 * orthonormal DCT-II table D[k][m] = sqrt(2 / M) cos(pi k (m + 1/2) / M), M = num_mels, formed in double on the host, rounded to float32.  Per frame
 *   d[m] = unit_db * (a[m] - b[m])
 *   0 bias = mean_m d[m]          1 l1  = mean_m |d[m]|          2 lsd  = sqrt(mean_m d[m]^2)
 *   3 mcd  = sqrt(0.5 * sum_{k = 1 ... n_cep} (sum_m D[k][m] d[m])^2)
 *   4 l1c  = mean_m |d[m] - bias_b|                              5 lsdc = sqrt(mean_m (d[m] - bias_b)^2)
 * with bias_b the mean of row b's bias over its frames: the level offset of the utterance, which the compensated distances 4 and 5 leave out.  mcd in
 * the usual units: for mels that are 20 log10 of an amplitude, d = (20 / ln 10) e with e the difference of the log amplitudes, so the DCT coefficients
 * are c_k = (20 / ln 10) dc_k, and the customary (10 / ln 10) sqrt(2 sum_k dc_k^2) = (10 / ln 10) (ln 10 / 20) sqrt(2 sum_k c_k^2) = sqrt(0.5 sum_k c_k^2).
 * Coefficient 0 (the level) is left out.  Outputs: per_frame[b][j][f], j = 0 ... 5 as numbered; summary[b] = the mean over the row's frames of each of
 * the six, then worst = max_f l1c; marks[b] = the frame of worst (the first maximum; -1 for an empty row), then the number of frames with
 * l1c > alarm_db.  An empty row gives zeros and -1.  Three passes over launch groups of 32 rows on the caller's stream, no host synchronisation: the
 * per-frame 0 ... 3; bias_b and the means of 0 ... 3; 4 and 5 with the remaining reductions.  Two reads of a and b in all, every one coalesced in
 * either layout (a workgroup stages 64 frames x num_mels through LDS and sums over channels from there in one order).  Reductions run in a fixed
 * order without atomics: the 6 F + 7 + 2 results of a row depend on that row's own frames alone -- not on B, its index, the launch group, the
 * pitches, the layouts, per_frame being asked for, or the run -- bit for bit.  The DCT table and the per-frame scratch [max_batch, 6, max_frames]
 * that stands in for a NULL per_frame are reserved at creation; no run allocates or synchronises, and frames travel as kernel arguments (the
 * host array is free when the call returns).  max_batch = 0 makes a validation-only handle that touches no device and refuses every run.
 * Validation before any device call: WN_E_ARG for a null pointer, a foreign abi_version, num_mels outside 1 ... 128, n_cep outside
 * [0, num_mels - 1], unit_db not finite or <= 0, alarm_db not finite or < 0, a negative max_batch or max_frames, B < 1, a negative frames[b];
 * WN_E_SHAPE for B > max_batch, frames[b] > max_frames, or a pitch (either input's, or out_pitch with per_frame given) smaller than the longest row. */
typedef struct wn_melcmp_config {
    int32_t abi_version;   /* = WN_ABI_VERSION */
    int32_t num_mels;      /* 1 ... 128 (the mel analysis' limit) */
    int32_t n_cep;         /* cepstral coefficients 1 ... n_cep of the distance, 0 <= n_cep <= num_mels - 1; 0: mcd is 0 */
    float   unit_db;       /* level units per unit of the inputs, finite, > 0 (normalised mels: -min_level_db / (2 max_abs_value) resp. / max_abs_value; 1 otherwise) */
    float   alarm_db;      /* finite, >= 0: a frame counts as alarmed when its l1c exceeds it */
    int32_t max_batch;     /* rows per call; 0: a validation-only handle that touches no device and refuses every run */
    int32_t max_frames;    /* frames per row (sizes the handle's per-frame scratch) */
} wn_melcmp_config;
typedef struct wn_melcmp wn_melcmp;
int  wn_melcmp_create(const wn_melcmp_config* cfg, wn_melcmp** out);
void wn_melcmp_destroy(wn_melcmp* h);
const char* wn_melcmp_last_error(const wn_melcmp* h);   /* NULL: text of the last failed create */
/* a, b: device float; frames: HOST int32 [B]; per_frame: device float [B, 6, out_pitch] or NULL; summary: device float [B, 7]; marks: device int32 [B, 2] */
int  wn_melcmp_run(wn_melcmp* h, const float* a, int32_t a_channels_first, int64_t a_pitch, const float* b, int32_t b_channels_first, int64_t b_pitch,
                   const int32_t* frames, int32_t B, float* per_frame, int64_t out_pitch, float* summary, int32_t* marks, void* stream);

/* ---- training summaries: histograms and per-tensor norms on the device ---------------------------
 * What the reference's add_train_stats writes every summary_interval steps (wavenet_vocoder/train.py:41-56: tf.summary.histogram of the decoded outputs,
 * the targets, the Gaussian head's means and log-scales and of the per-variable gradient norms, and max_gradient_norm = the largest of those norms) needs two
 * reductions: the histogram of a ragged batch and the L2 norm of every tensor of a flat buffer.  This module does both where the data is, with its own
 * handle and no context.  Histogram: TensorFlow's default summary buckets -- WN_HIST_BUCKETS ascending limits (wn_stats_hist_limits); a finite float32 x
 * belongs to the bucket of the first limit strictly greater than x widened to double -- plus summary[8] = {num, min, max, sum, sum_squares, n_nan, n_pos_inf,
 * n_neg_inf}; non-finite values enter their counter and nothing else, elements beyond lengths[b] and in the pitch gap are never read, an empty histogram
 * has min = max = 0.  Row b is x + b * pitch, so a pointer offset and a pitch address one channel of a [B, O, T] tensor.  Per-tensor statistics: a table of
 * disjoint (offset, count) runs of a flat float32 buffer, set once; per run out[nt, 4] = {sum of squares, max |x|, non-finite count, element count}, the
 * first two over the finite elements.  Every sum is a double in a fixed order (csrc/wn_stats.h): results are bit-identical from run to run and to the host
 * hooks; no float atomics, nothing waits across workgroups (a store pass and a sum pass per call).  Outputs are written whole: nothing to clear.  After
 * wn_stats_create nothing allocates and every run is asynchronous on `stream` (wn_stats_set_tensors copies its table synchronously).
 * Validation before any device call: WN_E_ARG for a null pointer, a foreign abi_version, a negative size (max_rows or max_tensors above 65535, max_time < 1
 * with max_rows > 0), B < 1, T < 1, nt < 1, a count <= 0, a negative offset, overlapping tensors; WN_E_SHAPE for B > max_rows, T > max_time, pitch < T,
 * nt > max_tensors, and for a tensor run on a validation-only handle; WN_E_STATE for wn_stats_tensors before wn_stats_set_tensors. */
#define WN_HIST_BUCKETS 1551
typedef struct wn_stats_config {
    int32_t abi_version;   /* = WN_ABI_VERSION */
    int32_t max_rows;      /* rows of a histogram call; 0: a validation-only handle that touches no device and refuses every run */
    int32_t max_time;      /* elements per row */
    int32_t max_tensors;   /* entries of the tensor table; 0: no tensor statistics */
} wn_stats_config;
typedef struct wn_stats wn_stats;
int  wn_stats_create(const wn_stats_config* cfg, wn_stats** out);
void wn_stats_destroy(wn_stats* h);
const char* wn_stats_last_error(const wn_stats* h);   /* NULL: text of the last failed create or host hook */
/* host only: the first min(cap, WN_HIST_BUCKETS) limits into out (out may be NULL with cap = 0); returns WN_HIST_BUCKETS */
int  wn_stats_hist_limits(double* out, int32_t cap);
/* x: device float, row b at x + b * pitch; lengths: DEVICE int32 [B] (held inside [0, T]) or NULL = every row T long; bucket: device int64 [WN_HIST_BUCKETS];
 * summary: device double [8] */
int  wn_stats_histogram(wn_stats* h, const float* x, int64_t pitch, const int32_t* lengths, int32_t B, int32_t T, int64_t* bucket, double* summary, void* stream);
/* offsets, counts: HOST int64 [nt] (floats into the flat buffer) */
int  wn_stats_set_tensors(wn_stats* h, const int64_t* offsets, const int64_t* counts, int32_t nt);
/* flat: device float; out: device double [nt, 4] */
int  wn_stats_tensors(wn_stats* h, const float* flat, double* out, void* stream);

/* ---- pitch check: F0 and voicing of a signal, and of a generated signal against a recording ----------------------------------------
 * A handle of its own, independent of the model context, like the mel analysis, the output stage and the reconstruction check: what an 80-band mel
 * cannot resolve -- pitch drift, octave jumps, voicing that flickers -- read off the waveforms themselves.  The estimator is YIN (de Cheveigne &
 * Kawahara 2002, steps 2 ... 5) on frames aligned with the mel frames: a signal of n samples has F = 1 + n / hop frames, and with L = window + tau_max
 * frame f covers the signal indices [f hop - L / 2, f hop - L / 2 + L), zeros outside [0, n): x_0 ... x_{L-1}.
 *   d(tau)  = sum_{j = 0 ... window-1} (x_j - x_{j+tau})^2    tau = 1 ... tau_max; float32, one accumulator, j ascending, e = x_j - x_{j+tau}; acc = fma(e, e, acc)
 *   c(tau)  = sum_{k = 1 ... tau} d(k)                         float32, tau ascending
 *   d'(0)   = 1;  d'(tau) = c(tau) > 0 ? (d(tau) tau) / c(tau) : 1
 * The direct form of d on purpose: all terms are non-negative, so every d'(tau) is within (window + tau_max + 8) 2^-24, relative, of its exact value; the
 * energy-minus-autocorrelation form has no such bound.  Pick over tau in [tau_min, tau_max - 1]: the first tau with d'(tau) < threshold, then walk while
 * tau + 1 <= tau_max - 1 and d'(tau + 1) < d'(tau).  If there is one the frame is voiced: with a = d'(tau - 1), b = d'(tau), c = d'(tau + 1), den = a - 2 b + c,
 * delta = den > 0 ? 0.5 (a - c) / den : 0,  f0 = sample_rate / (tau + delta),  ap = b.  Otherwise it is unvoiced: f0 = 0, ap = min d' over the range.  No
 * energy gate, no smoothing, no octave post-processing; digital silence is unvoiced with ap = 1.  Cells of frames >= a row's F keep the caller's bytes.
 * A frame's results depend on that row's samples alone -- not on B, the row's index, ld, F_max, which outputs are asked for, or the run -- bit for bit.
 * wn_pitch_compare: a reference track a against a generated track b over the first frames[b] frames of row b, a frame being voiced when its f0 > 0; one
 * float32 row of 9: frames, voiced_a, voiced_b, both, vuv_error (share of frames whose voiced flags differ), gpe (share of both-voiced frames with
 * |f_b / f_a - 1| > 0.2), f0_rmse_cents and f0_bias_cents (over the both-voiced frames, of 1200 log2(f_b / f_a) in double), f0_fine_rmse_cents (the same
 * RMSE over the both-voiced frames that are not gross); an empty denominator gives 0.  Sums are doubles added in frame order, no atomics.
 * The handle holds no device memory (a tile's signal span and its d' table live in LDS): creation touches no device, no call allocates or synchronises,
 * lengths and frames travel as kernel arguments (the host arrays are free when the call returns).
 * Validation before any device call: WN_E_ARG for a null pointer, a foreign abi_version, sample_rate < 1, hop < 1, window < 1, tau_min < 2,
 * tau_max <= tau_min + 1, threshold outside (0, 1], max_batch < 1, a negative size, B < 1; WN_E_UNSUPPORTED when one tile's span, 7 hop + window + tau_max
 * floats, and its table, 8 (tau_max + 1), exceed the 64 KiB of LDS the kernel is built for; WN_E_SHAPE for B > max_batch, F_max beyond the frames of
 * max_samples or below a row's, lengths[b] > ld or > max_samples, frames[b] > pitch or beyond the frames of max_samples. */
typedef struct wn_pitch_config {
    int32_t abi_version;   /* = WN_ABI_VERSION */
    int32_t sample_rate;   /* Hz */
    int32_t hop;           /* samples between frames: the mel analysis' hop_size */
    int32_t window;        /* W: terms of the difference function */
    int32_t tau_min;       /* >= 2: sample_rate / the highest f0 */
    int32_t tau_max;       /* > tau_min + 1: ceil(sample_rate / the lowest f0) */
    float   threshold;     /* in (0, 1]: a lag whose d' falls below it is a candidate */
    int32_t max_batch;     /* rows per call, >= 1 */
    int64_t max_samples;   /* samples per row */
} wn_pitch_config;
typedef struct wn_pitch wn_pitch;
int  wn_pitch_create(const wn_pitch_config* cfg, wn_pitch** out);
void wn_pitch_destroy(wn_pitch* h);
const char* wn_pitch_last_error(const wn_pitch* h);   /* NULL: text of the last failed create or host hook */
/* 1 + n_samples / hop; WN_E_ARG for a NULL handle or n_samples < 0 (host only) */
int64_t wn_pitch_num_frames(const wn_pitch* h, int64_t n_samples);
/* frames one workgroup takes (8): tests place row lengths around its multiples */
int  wn_pitch_frame_tile(const wn_pitch* h);
/* wav: device float [B, ld], row b holds lengths[b] <= ld samples (HOST int32 [B], as wn_mel_run); f0: device float [B, F_max]; ap: device float
 * [B, F_max] or NULL; dprime: device float [B, F_max, tau_max + 1] or NULL */
int  wn_pitch_run(wn_pitch* h, const float* wav, int64_t ld, const int32_t* lengths, int32_t B, int32_t F_max, float* f0, float* ap, float* dprime, void* stream);
/* f0_a, f0_b: device float [B, pitch]; frames: HOST int32 [B]; table: device float [B, 9] */
int  wn_pitch_compare(wn_pitch* h, const float* f0_a, const float* f0_b, int64_t pitch, const int32_t* frames, int32_t B, float* table, void* stream);

/* ---- spectral denoiser (csrc/wn_denoise.hip) ----------------------------------------------------
 * The bias denoiser of sampled vocoders on decoded float samples: STFT with a periodic Hann window of n_fft at hop (frames as wn_mel: F = 1 + n / hop,
 * frame f centred on f hop, zeros outside [0, n)), |X| of every bin lowered by strength x profile[bin] and clamped at zero with the phase kept, inverse
 * transform, synthesis window, overlap-add divided by the window-square sum of the covering frames (ascending f).  The profile is the mean |X| per bin
 * over the frames of some signal whose window lies wholly inside it -- fitted on the device (wn_denoise_fit) or given (wn_denoise_set_profile).  A
 * handle of its own, independent of wn_ctx.  All device memory -- both tables, the profile, two frame workspaces of max_batch x frames(max_samples) x
 * n_fft floats, the partial sums of fit -- is reserved by wn_denoise_create; fit and run allocate nothing and never synchronise; lengths travel as
 * kernel arguments (the host arrays are free when the call returns); no atomics, every sum in an order that depends only on (n_fft, hop) and the
 * sample's own row, so a row's output bits do not depend on the batch, the row index or the pitches.
 * Validation before any device call, in this order.  WN_E_ARG: a null pointer, a foreign abi_version, a negative size, B < 1, strength negative or not
 * finite, a negative or non-finite profile entry.  WN_E_STATE: run / get_profile before any profile was fitted or set.  WN_E_SHAPE: n_fft odd or below 8,
 * hop outside [1, n_fft / 4], B > max_batch, lengths[b] above a pitch or above max_samples, fit with no frame wholly inside any row.  WN_E_UNSUPPORTED:
 * n_fft not a multiple of 32 or above 4096 (the inverse product runs in whole 32-column groups; the span of a 32-frame tile, 31 hop + n_fft floats, must
 * fit the LDS): (1024, 256), (2048, 512) and (4096, 1024) are admitted. */
typedef struct wn_denoise_config {
    int32_t abi_version;   /* = WN_ABI_VERSION */
    int32_t n_fft;         /* window and transform length */
    int32_t hop;           /* samples between frames, 1 ... n_fft / 4 */
    int32_t max_batch;     /* rows per call; 0: geometry-only handle (validation, num_frames, a host copy of a set profile): no device is touched */
    int64_t max_samples;   /* samples per row */
} wn_denoise_config;
typedef struct wn_denoise wn_denoise;
int  wn_denoise_create(const wn_denoise_config* cfg, wn_denoise** out);
void wn_denoise_destroy(wn_denoise* h);
const char* wn_denoise_last_error(const wn_denoise* h);   /* NULL: text of the last failed create or host hook */
/* 1 + n / hop; WN_E_ARG for a NULL handle or n < 0 (host only) */
int64_t wn_denoise_num_frames(const wn_denoise* h, int64_t n);
/* wav: device float [B, ld], row b holds lengths[b] <= ld samples (HOST int32 [B]).  Sets the handle's profile: per (row, tile of 32 frames) partial sums in
 * float32, frames ascending, then (row, tile) ascending in double, divided by the frame count and rounded to float32 */
int  wn_denoise_fit(wn_denoise* h, const float* wav, int64_t ld, const int32_t* lengths, int32_t B, void* stream);
/* profile: HOST float [1 + n_fft / 2]; its values travel as kernel arguments: the array is free when the call returns, nothing synchronises */
int  wn_denoise_set_profile(wn_denoise* h, const float* profile, void* stream);
/* profile: HOST float [1 + n_fft / 2].  SYNCHRONISES the stream: the only call of the handle that does */
int  wn_denoise_get_profile(wn_denoise* h, float* profile, void* stream);
/* in: device float [B, in_pitch]; out: device float [B, out_pitch], in == out allowed.  Elements of an out row beyond lengths[b] keep the caller's bytes;
 * lengths[b] = 0 writes nothing */
int  wn_denoise_run(wn_denoise* h, const float* in, int64_t in_pitch, const int32_t* lengths, int32_t B, float strength, float* out, int64_t out_pitch, void* stream);

/* ---- streaming spectral denoiser (csrc/wn_denoise_stream.hip) -----------------------------------
 * The denoiser above on rows that arrive push by push (the playable chunks of streams and slot sessions): a row's emitted samples, concatenated over its
 * pushes, are BIT-IDENTICAL to wn_denoise_run of the whole row, however the row is cut.  A handle of its own, independent of wn_ctx and of wn_denoise.
 * With H = n_fft / 2, S the samples a row was given since its restart and E those it has emitted, the emit rule depends on (n_fft, hop, S, final) alone:
 *   E = S when final;  otherwise E = max(0, (floor((S - H) / hop) + 1) hop - H)   (floor towards -inf; 0 for S < H)
 * so S - n_fft < E <= S - n_fft + hop whenever E > 0: the lag is below n_fft samples.  Frame f is analysed once f hop + H <= S, or when the row is final
 * (zeros beyond the end, F = 1 + S / hop frames, as wn_denoise_run pads).  Per row the handle keeps the input tail (the < n_fft decoded samples the next
 * frame still needs, double-buffered: a push reads one half and writes the other) and a ring of R = ceil(n_fft / hop) + (max_push + H) / hop + 2 windowed
 * frames: those that still cover unemitted samples and those one push can add.  A push is two launches per group of 64 rows: the tile kernel (one
 * workgroup per row and 32 new frames: stages tail + decoded new samples in LDS, the forward product, shrink and inverse product of wn_denoise_run in the
 * same instruction order, frames into the ring, the new tail) and the gather kernel (out[E_old ... E_new) from the ring, frames ascending, one division).
 * All device memory is reserved by create; a push allocates nothing, uses no atomics and never synchronises; the row counters live on the host and travel
 * as kernel arguments.  Calls on one handle belong on one stream at a time.
 * Validation before any device call, as wn_denoise's.  WN_E_ARG: a null pointer, a foreign abi_version, a negative size, in_type outside 0 ... 2, B < 1,
 * a negative n[b] or pitch, strength negative or not finite, a bad profile entry.  WN_E_STATE: a push before any profile; a push (n[b] > 0 or final[b])
 * on a row that ended without restart[b].  WN_E_SHAPE: the geometry rules of wn_denoise, B > max_rows, n[b] > max_push or > in_pitch, out_pitch below some
 * n_out[b], a row beyond 2^31 - 1 samples since its restart.  WN_E_UNSUPPORTED: the geometry limits of wn_denoise, and a reserve (tables, tails, rings and
 * the tiles' spectrum rows: max_rows x (2 n_fft + R n_fft + 32 ceil(((max_push + H) / hop + 2) / 32) n_fft) floats) above 4 GiB. */
typedef struct wn_denoise_stream_config {
    int32_t abi_version;   /* = WN_ABI_VERSION */
    int32_t n_fft;         /* as wn_denoise_config */
    int32_t hop;
    int32_t max_rows;      /* rows of carried state; 0: geometry-only handle (validation, ready, the counters of a push): no device is touched */
    int32_t max_push;      /* most samples per row in one push, >= 1 */
    int32_t in_type;       /* as wn_post_config: 0 float waveform, 1 float mu-law, 2 int32 class ids; decoded while staging (wn_post_decode) */
} wn_denoise_stream_config;
typedef struct wn_denoise_stream wn_denoise_stream;
int  wn_denoise_stream_create(const wn_denoise_stream_config* cfg, wn_denoise_stream** out);
void wn_denoise_stream_destroy(wn_denoise_stream* h);
const char* wn_denoise_stream_last_error(const wn_denoise_stream* h);   /* NULL: text of the last failed create or host hook */
/* profile: HOST float [1 + n_fft / 2], as wn_denoise_set_profile (kernel arguments, nothing synchronises) */
int  wn_denoise_stream_set_profile(wn_denoise_stream* h, const float* profile, void* stream);
/* the fitted or set profile of a wn_denoise of the same n_fft (WN_E_SHAPE otherwise; WN_E_STATE if it has none), copied device to device on `stream`
 * behind the fit enqueued there: nothing synchronises */
int  wn_denoise_stream_take_profile(wn_denoise_stream* h, const wn_denoise* src, void* stream);
/* E of the rule above (host only); WN_E_ARG for a NULL handle or S < 0 */
int64_t wn_denoise_stream_ready(const wn_denoise_stream* h, int64_t S, int32_t final);
/* in: device [B, in_pitch] elements of in_type, row b's next n[b] samples (never read beyond n[b]; NULL allowed when every n[b] is 0); out: device float
 * [B, out_pitch], row b receives n_out[b] samples, elements beyond keep the caller's bytes.  n, restart, final (either may be NULL: none), n_out: HOST
 * int32 [B]; n_out is computed from the counters and written before the call returns.  restart[b]: row b starts at S = E = 0 before it consumes its
 * samples (a slot reopened inherits nothing).  final[b]: the row's utterance ends, everything left is flushed, and its next push must restart it.  A row
 * with n[b] = 0 that is neither restarted nor final is left alone.  A failed call changes no row. */
int  wn_denoise_stream_push(wn_denoise_stream* h, const void* in, int64_t in_pitch, const int32_t* n, const int32_t* restart, const int32_t* final, int32_t B,
                            float strength, float* out, int64_t out_pitch, int32_t* n_out, void* stream);

/* ---- sample-rate conversion (csrc/wn_resample.hip) ----------------------------------------------
 * Rows of float32 samples from sr_in to sr_out by the rational factor L / M (g = gcd(sr_in, sr_out), L = sr_out / g, M = sr_in / g), whole rows (wn_resample_run)
 * or push by push (wn_resample_push: row = slot, the playable chunks of streams and slot sessions).  A handle of its own, independent of wn_ctx.
 * The filter is a Kaiser-windowed sinc in closed form, h(t) = rolloff sinc(rolloff t) I0(beta sqrt(1 - (t / zeros)^2)) / I0(beta) for |t| < zeros, else 0; with
 * s = min(1, L / M), output m of a row of n samples is
 *   y[m] = s sum_k x[k] h(s (m M / L - k)),  x = 0 outside [0, n),  m < n_out = ceil(n L / M)                        (the last sample computed, not zero-filled)
 * evaluated in polyphase form: W = ceil(zeros max(L, M) / L), T = 2 W taps, k0 = floor(m M / L), p = (m M) mod L,
 *   y[m] = sum_{j < T} C[p][j] x[k0 - W + 1 + j],  C[p][j] = s h(s (p / L + W - 1 - j))
 * C [L][T] is evaluated in double on the host EXACTLY at the polyphase positions and rounded once to float32 (no interpolation from a sampled table: the
 * result differs from resampy's kaiser_best, whose design values zeros = 64, beta = 14.769656459379492, rolloff = 0.9475937167399596 are the usual choice,
 * by that table's interpolation error).  One float32 accumulator per output from 0, T fmaf in ascending j, taps outside the row read 0.0f and are never
 * skipped: an output's bits depend on (L, M, zeros, beta, rolloff), m and the row's samples alone -- not on the batch, the row index, the pitches or how the
 * row was cut into pushes -- and equal the plain loop of wn_test_resample_host.  sr_in == sr_out (L = M = 1) does not filter: W = 0 and the bits are copied.
 * Streaming: S inputs given to a row since its restart, E outputs emitted.  Final: E = ceil(S L / M).  Otherwise E = max(0, ceil((S - W) L / M)): the lag is at
 * most W inputs (177, about 8 ms, for 22 050 -> 8 000 Hz).  Per row the handle keeps the counters on the host and at most 2 W - 1 inputs on the device,
 * double-buffered.  All device memory (the table, the tails) is reserved by create; no call allocates, uses atomics or synchronises.  Calls on one handle
 * belong on one stream at a time.
 * Validation before any device call.  WN_E_ARG: a null pointer, a foreign abi_version, negative max_rows / max_in / lengths / pitches, B < 1, sr_in or sr_out
 * below 1, zeros < 1, rolloff outside (0, 1], beta negative or not finite.  WN_E_SHAPE: B > max_rows, a row longer than max_in or its pitch, out_pitch below
 * some row's outputs, a row beyond 2^31 - 1 samples since its restart.  WN_E_STATE: a push (n[b] > 0 or final[b]) on a row that ended without restart[b].
 * WN_E_UNSUPPORTED: a table L x T above 4 Mi floats (22 050 -> 8 000 needs 56 640), more than 12 288 inputs under a block of 64 outputs, beta above 256. */
typedef struct wn_resample_config {
    int32_t abi_version;   /* = WN_ABI_VERSION */
    int32_t max_rows;      /* rows of one call and of carried state; 0: geometry-only handle (validation, num_out, ready, taps): no device is touched */
    int32_t max_in;        /* most input samples per row in one call; >= 1 when max_rows > 0 (0 on a geometry-only handle or in a hook: no limit) */
    int32_t sr_in;         /* >= 1 */
    int32_t sr_out;        /* >= 1 */
    int32_t zeros;         /* zero crossings of the prototype on each side, >= 1 */
    double  beta;          /* Kaiser window shape, finite, 0 ... 256 */
    double  rolloff;       /* cutoff as a share of the lower Nyquist frequency, in (0, 1] */
} wn_resample_config;
typedef struct wn_resample wn_resample;
int  wn_resample_create(const wn_resample_config* cfg, wn_resample** out);
void wn_resample_destroy(wn_resample* h);
const char* wn_resample_last_error(const wn_resample* h);   /* NULL: text of the last failed create or host hook */
/* ceil(n L / M) and E of the rule above (host only); WN_E_ARG for a NULL handle or an n / S outside [0, 2^31 - 1] */
int64_t wn_resample_num_out(const wn_resample* h, int64_t n);
int64_t wn_resample_ready(const wn_resample* h, int64_t S, int32_t final);
/* the plan: any of L, M, W may be NULL */
int  wn_resample_taps(const wn_resample* h, int32_t* L, int32_t* M, int32_t* W);
/* whole ragged rows.  in: device float [B, in_pitch], row b holds lengths[b] samples (HOST int32 [B]); out: device float [B, out_pitch], row b receives
 * ceil(lengths[b] L / M) samples, elements beyond keep the caller's bytes.  Neither reads nor writes the carried state of a push. */
int  wn_resample_run(wn_resample* h, const float* in, int64_t in_pitch, const int32_t* lengths, int32_t B, float* out, int64_t out_pitch, void* stream);
/* in: device float [B, in_pitch], row b's next n[b] samples (never read beyond n[b]; NULL allowed when every n[b] is 0); out: device float [B, out_pitch], row b
 * receives n_out[b] samples, elements beyond keep the caller's bytes.  n, restart, final (either may be NULL: none), n_out: HOST int32 [B]; n_out is computed
 * from the counters and written before the call returns.  restart[b]: row b starts at S = E = 0 before it consumes its samples.  final[b]: the row ends,
 * everything left is flushed, and its next push must restart it.  A row with n[b] = 0 that is neither restarted nor final is left alone.  A failed call
 * changes no row. */
int  wn_resample_push(wn_resample* h, const float* in, int64_t in_pitch, const int32_t* n, const int32_t* restart, const int32_t* final, int32_t B, float* out,
                      int64_t out_pitch, int32_t* n_out, void* stream);

/* ---- streaming mel analysis (csrc/wn_mel_stream.hip) --------------------------------------------
 * wn_mel_run on rows that arrive push by push (row = slot: the front end of a live vocoder).  A handle of its own; additions only, WN_ABI_VERSION unchanged.
 * A row's frames, concatenated over its pushes, are bit-identical to wn_mel_run of the whole row with the same gain and pre-emphasis, however the row was cut:
 * every frame's sums run in wn_mel's order (csrc/wn_mel.h) whichever tile it falls into.
 * Geometry as wn_mel: off = (n_fft - win_size) / 2, Hl = n_fft / 2 - off, Hr = win_size - Hl; frame f reads y[f hop - Hl ... f hop + Hr), y = 0 outside the row,
 * y[s] = gain (x[s] - preemphasis x[s - 1]) in three separately rounded operations, x[-1] = 0.
 * Rule of readiness (beside E of wn_denoise_stream): a row that has consumed S samples since its restart has had its frames f with f hop + Hr <= S analysed,
 * (S - Hr) / hop + 1 of them (0 for S < Hr); when the row is final, all 1 + S / hop frames, zeros beyond the end, as wn_mel_run pads.  wn_mel_stream_ready
 * returns that count; the frames lag the samples by Hr (550 samples, about 25 ms, at the default 2048 / 1100 / 275).
 * Per row the handle keeps, all reserved by create: the analysed-domain tail y[max(0, F hop - Hl), S) the next frame still needs (fewer than win_size samples,
 * double-buffered on the device: a push reads one half and writes the other), the raw last sample x[S - 1] for the pre-emphasis, the gain latched at the
 * restart, and the counters S and F on the host (they travel as kernel arguments).  No call allocates, uses atomics or synchronises; rows go in groups of 64
 * per launch; calls on one handle belong on one stream at a time.  cfg->max_batch and cfg->max_samples are ignored.  max_rows = 0 makes a geometry-only
 * handle: no device is touched, wn_mel_stream_ready works and wn_mel_stream_push refuses every B.
 * Validation before any device call.  WN_E_ARG: a null pointer, a foreign abi_version, negative max_rows / n[b] / pitches, max_push < 1, B < 1, a gain that is
 * not finite, and wn_mel's.  WN_E_STATE: a push (n[b] > 0 or final[b]) on a row that ended without restart[b].  WN_E_SHAPE: wn_mel's geometry rules,
 * B > max_rows, n[b] > max_push or > in_pitch, out_pitch below some n_out[b], a row beyond 2^31 - 1 samples since its restart.  WN_E_UNSUPPORTED: the limits
 * of wn_mel: num_mels > 128, n_fft > 65536, 31 hop_size + win_size floats beyond the 160 KiB LDS. */
typedef struct wn_mel_stream wn_mel_stream;
int  wn_mel_stream_create(const wn_mel_config* cfg, const float* mel_basis, int32_t max_rows, int32_t max_push, wn_mel_stream** out);
void wn_mel_stream_destroy(wn_mel_stream* h);
const char* wn_mel_stream_last_error(const wn_mel_stream* h);   /* NULL: text of the last failed create or host hook */
/* frames analysed of a row at S (host only); WN_E_ARG for a NULL handle or an S outside [0, 2^31 - 1] */
int64_t wn_mel_stream_ready(const wn_mel_stream* h, int64_t S, int32_t final);
/* in: device float [B, in_pitch], row b's next n[b] samples (never read beyond n[b]; NULL allowed when every n[b] is 0); out: device float
 * [B, out_pitch, num_mels] (channels_first = 0) or [B, num_mels, out_pitch] (1), row b receives n_out[b] frames, elements beyond keep the caller's bytes.
 * n, restart, final, n_out: HOST int32 [B]; gain: HOST float [B]; restart, final and gain may be NULL.  n_out is computed from the counters and written before
 * the call returns.  restart[b]: row b starts at S = F = 0 before it consumes its samples, inherits nothing, and latches gain[b] (1 with a NULL gain) for its
 * life; gain[b] is read nowhere else.  final[b]: the row ends, its remaining frames are flushed, and its next push must restart it.  A row with n[b] = 0 that
 * is neither restarted nor final is left alone.  A failed call changes no row. */
int  wn_mel_stream_push(wn_mel_stream* h, const float* in, int64_t in_pitch, const int32_t* n, const int32_t* restart, const int32_t* final, const float* gain, int32_t B,
                        float* out, int64_t out_pitch, int32_t channels_first, int32_t* n_out, void* stream);

/* ---- Griffin-Lim: mel -> signal without a model (csrc/wn_griffin.hip) ----------------------------
 * The reference's inv_mel_spectrogram / _griffin_lim (datasets/audio.py:97-112, 151-161) up to the de-emphasis: the baseline a trained vocoder has to beat
 * on the same mels.  A handle of its own, independent of wn_ctx; additions only, WN_ABI_VERSION unchanged.  Geometry: n_fft, win_size <= n_fft, hop; the
 * window is a periodic Hann of win_size centred in n_fft, frames as those of the mel analysis -- frame f centred on f hop, zeros outside the row --, the inverse is librosa's istft
 * (windowed inverse DFT, overlap-add, division by the window-square sum of the covering frames, n_fft / 2 trimmed at both ends): a row of F frames is
 * n = hop (F - 1) samples.  Magnitudes S [F, 1 + n_fft / 2] come from a normalised mel -- the inverse of the four _normalize variants of wn_mel,
 * 10^((D + ref_level_db) / 20), ^(1 / magnitude_power), the product with pinv(mel_basis) (mels ascending), max(1e-10, .), ^power -- or are given.
 * A run: the start y0 = ISTFT(S e^{2 pi i u}) from caller-given uniforms u (or zero phase, or a caller-given y0), then `iters` iterations
 * y <- ISTFT(S phase(STFT(y))); an exactly zero bin takes the phase (1, 0).  Exact fp32 products (the fp32 matrix instruction) summed in orders that depend
 * on the geometry and the sample's own row alone: two runs, and a row alone or inside any batch, are bit-identical; run(a) then a continuation of b equals
 * run(a + b).  All device memory -- the two tables, pinv, the magnitudes, the spectrum and frame workspaces and y -- is reserved by wn_griffin_create; a run
 * allocates nothing and never synchronises; frame counts travel as kernel arguments (the host array is free when the call returns).  max_batch = 0 makes a
 * geometry-only handle.
 * Validation before any device call.  WN_E_ARG: a null pointer, a foreign abi_version, a negative size or pitch, num_mels outside [0, 512], magnitude_power
 * or power not finite or <= 0, B < 1, iters < 0, a src_kind outside 0 ... 2, a mel input on a handle created without pinv, unknown flags.  WN_E_STATE: a
 * continuation before any run.  WN_E_SHAPE: n_fft odd or below 8, win_size outside [4, n_fft], hop outside [1, win_size / 4] (the range that keeps every
 * trimmed sample's window-square sum positive), frames[b] < 2, B > max_batch, frames[b] above F_max or max_frames, a row longer than a pitch.
 * WN_E_UNSUPPORTED: n_fft not a multiple of 32 or above 4096. */
typedef struct wn_griffin_config {
    int32_t abi_version;   /* = WN_ABI_VERSION */
    int32_t n_fft, win_size, hop;
    int32_t num_mels;      /* 0: magnitudes only */
    float   magnitude_power, power;                               /* hparams.py magnitude_power, power (1.5) */
    float   min_level_db, ref_level_db, max_abs_value;
    int32_t signal_normalization, allow_clipping, symmetric_mels; /* as wn_mel_config */
    int32_t max_batch;     /* rows per call; 0: geometry-only handle */
    int32_t max_frames;    /* frames per row */
} wn_griffin_config;
typedef struct wn_griffin wn_griffin;
#define WN_GRIFFIN_SRC_MEL 0        /* src: device float [B, F_max, num_mels] */
#define WN_GRIFFIN_SRC_MEL_CF 1     /* [B, num_mels, F_max] */
#define WN_GRIFFIN_SRC_MAG 2        /* [B, F_max, 1 + n_fft / 2], used as is */
#define WN_GRIFFIN_CONTINUE 1       /* flags: carry on from the handle's y and magnitudes */
/* pinv: HOST float [1 + n_fft / 2, num_mels] (np.linalg.pinv(mel_basis)), or NULL for a handle that takes magnitudes only */
int  wn_griffin_create(const wn_griffin_config* cfg, const float* pinv, wn_griffin** out);
void wn_griffin_destroy(wn_griffin* h);
const char* wn_griffin_last_error(const wn_griffin* h);   /* NULL: text of the last failed create or host hook */
/* hop (frames - 1); WN_E_ARG for a NULL handle or frames < 1 (host only) */
int64_t wn_griffin_num_samples(const wn_griffin* h, int64_t frames);
/* src: as src_kind says; frames: HOST int32 [B].  The start: y0 (device float [B, y0_pitch]) if given, else u (device float [B, F_max, 1 + n_fft / 2] in
 * [0, 1)) if given, else zero phase.  Then `iters` iterations.  out: device float [B, out_pitch] or NULL (the result stays in the handle); row b receives
 * hop (frames[b] - 1) samples, elements beyond keep the caller's bytes.  flags = WN_GRIFFIN_CONTINUE: src, src_kind, F_max, frames, B, u, y0 are ignored and
 * `iters` further iterations run on the rows of the handle's last run. */
int  wn_griffin_run(wn_griffin* h, const float* src, int32_t src_kind, int32_t F_max, const int32_t* frames, int32_t B, const float* u, const float* y0,
                    int64_t y0_pitch, int32_t iters, int32_t flags, float* out, int64_t out_pitch, void* stream);

/* ---- alignment check (csrc/wn_align.hip): MCD along a dynamic-time-warping path, and the path itself -------------------------------------------
 * The reconstruction and pitch checks need frame-aligned signals.  A generated utterance whose mels were PREDICTED (synthesize.py --mels_dir) has another
 * length and timing than any recording; this module aligns the two mel-spectrograms by dynamic time warping over their cepstral distance and reports the
 * mel-cepstral distortion along the path (MCD-DTW) with the path and the two frame maps, so that F0 can be compared along the same path.  A handle of its
 * own, independent of wn_ctx; additions only, WN_ABI_VERSION unchanged.  a, b: device float32, each channels-first [B, num_mels, pitch] or channels-last
 * [B, pitch, num_mels] as wn_melcmp_run takes them; row r has frames_a[r] resp. frames_b[r] frames (Fa, Fb), each >= 1; elements beyond are never read
 * into a result.  Arithmetic, all float32, every step rounded on its own (csrc/wn_align.h):
 *   cepstra     u[m] = unit_db * x[m];  c[k] = sum_m D[k][m] u[m], k = 1 ... n_cep, fused multiply-adds in channel order, D the table of wn_melcmp
 *   cell cost   cost(i, j) = sqrt(0.5 * sum_k (ca[i][k] - cb[j][k])^2): e = ca - cb, acc = fma(e, e, acc), k ascending -- the MCD of the frame pair in dB
 *   band        (i, j) is admissible iff band == 0 or |i Fb - j Fa| <= band * max(Fa, Fb) (int64); inadmissible cells count as +inf.  For band >= 1
 *               the staircase j = floor(i Fb / Fa) (or its transpose) lies inside the band, so (0, 0) and (Fa-1, Fb-1) are always connected
 *   recurrence  Dm(0, 0) = cost(0, 0);  Dm(i, j) = cost(i, j) + min(Dm(i-1, j-1), Dm(i-1, j), Dm(i, j-1)), one rounded add; the predecessor is the smallest
 *               candidate, ties to the first of diagonal, (i-1, j), (i, j-1); cells outside the matrix or the band are never chosen
 *   path        back-trace from (Fa-1, Fb-1) to (0, 0), at most Fa + Fb - 2 steps whose indices cannot leave the matrix whatever the values (non-finite
 *               inputs give an unspecified but valid path), delivered in FORWARD order
 * Outputs (device; elements beyond a row's extent keep the caller's bytes): path int32 [B, 2, path_pitch] (i then j of the n_path cells), map_ab int32
 * [B, map_a_pitch] the largest j paired with i, map_ba int32 [B, map_b_pitch] the largest i paired with j -- each may be NULL -- and summary float
 * [B, 7]: Fa, Fb, n_path, total = Dm(Fa-1, Fb-1), mcd_dtw = (the sum of the path's costs as doubles in path order) / n_path, the share of
 * non-diagonal steps, max_p |i_p Fb - j_p Fa| / max(Fa, Fb).  A row's results depend on that row alone -- not on B, its index, the pitches, the
 * layouts, which outputs are asked for, or the run -- bit for bit.  Four launches per group of 32 rows on the caller's stream (cepstra, cost matrix,
 * recurrence with one workgroup per row walking 64 x 64 blocks along block anti-diagonals, back-trace); nothing waits across workgroups.  The cepstra,
 * the cost matrix [max_batch, max_frames_a, max_frames_b] and the 2-bit directions are reserved at creation; no run allocates or synchronises, and the
 * frame counts travel as kernel arguments (the host arrays are free when the call returns).  max_batch = 0 makes a validation-only handle that
 * touches no device and refuses every run.
 * Validation before any device call: WN_E_ARG for a null pointer (a, b, frames_a, frames_b, summary), a foreign abi_version, num_mels outside 1 ... 128,
 * n_cep outside [1, num_mels - 1], unit_db not finite or <= 0, band outside [0, 2^20], a negative max_batch / max_frames_a / max_frames_b (or below 1 with
 * max_batch > 0), B < 1, a frame count < 1; WN_E_UNSUPPORTED from wn_align_create for max_frames_a or max_frames_b above 4096 or
 * max_batch x max_frames_a x max_frames_b above 2^27 cells (the reserve limit); WN_E_SHAPE for B > max_batch, frames above the maxima, path_pitch below
 * the longest possible path max_r (Fa + Fb - 1), a map pitch or an input pitch below the longest row. */
typedef struct wn_align_config {
    int32_t abi_version;   /* = WN_ABI_VERSION */
    int32_t num_mels;      /* 1 ... 128 */
    int32_t n_cep;         /* cepstral coefficients 1 ... n_cep of the cost, 1 <= n_cep <= num_mels - 1 */
    float   unit_db;       /* as wn_melcmp_config */
    int32_t band;          /* 0: every cell admissible; r >= 1: |i Fb - j Fa| <= r max(Fa, Fb) */
    int32_t max_batch;     /* rows per call; 0: a validation-only handle that touches no device and refuses every run */
    int32_t max_frames_a;  /* frames per row of a and of b: size the handle's scratch */
    int32_t max_frames_b;
} wn_align_config;
typedef struct wn_align wn_align;
int  wn_align_create(const wn_align_config* cfg, wn_align** out);
void wn_align_destroy(wn_align* h);
const char* wn_align_last_error(const wn_align* h);   /* NULL: text of the last failed create or host hook */
/* rows and columns of one block of the recurrence (64): tests place frame counts around its multiples */
int  wn_align_tile(const wn_align* h);
/* a, b: device float; frames_a, frames_b: HOST int32 [B]; path, map_ab, map_ba: device int32 or NULL; summary: device float [B, 7] */
int  wn_align_run(wn_align* h, const float* a, int32_t a_channels_first, int64_t a_pitch, const float* b, int32_t b_channels_first, int64_t b_pitch,
                  const int32_t* frames_a, const int32_t* frames_b, int32_t B, int32_t* path, int64_t path_pitch, int32_t* map_ab, int64_t map_a_pitch,
                  int32_t* map_ba, int64_t map_b_pitch, float* summary, void* stream);

/* ---- introspection ------------------------------------------------------------------------------ */
int64_t wn_workspace_bytes(const wn_ctx* ctx);
/* name of the kernel that dominates training time (bench.py's roofline line names it) */
const char* wn_dominant_kernel_name(void);

/* ================================================================================================
 * WN_TEST_HOOKS -- NOT part of the drop-in surface.  Entry points used only by tests/, bench.py and tools/ to look inside a
 * context; a reference-side binding has no use for them.  Compile callers with -DWN_NO_TEST_HOOKS to hide the declarations.
 * ================================================================================================ */
#ifndef WN_NO_TEST_HOOKS
/* copy an internal activation buffer of the last step to `out` as fp32 ("X","U","TS","DZ","R1","H2","DY","DSKIP","DPRE1","GX0",
 * "GX1","cbt" are bf16 [rows][channels]; "YHAT","DC","CUP" fp32).  "GX" with layer 0 ... L is d L / d h_layer as the backward chain
 * keeps it (layer L: the zero-filled top), "XD" with layer 0 ... L-1 the dropout-applied conv input (the same buffer as "X" when
 * dropout is 0); a layer outside these ranges is WN_E_ARG.  An fp32-mode context (compute_dtype = WN_COMPUTE_F32) keeps fp32 buffers instead: "X", "U" and
 * "Z" (the gate pre-activations [rows][gate_channels]) per layer 0 ... L-1, "SK" (ReLU of the skip sum) and "H1" (ReLU of final_convolution_1), both
 * [rows][skip_out_channels] with layer 0; they persist after the forward.
 * The weight path (fp32, `layer` ignored, n above the buffer's length is WN_E_ARG, WN_E_STATE before wn_pack_weights; all but "DEFF" also on
 * inference-only contexts): "PARAMS" the context's EFFECTIVE parameter copy (n_params floats in the effective layout: the raw tensors without
 * the gains, each 8-float aligned, in wn_tensor_info order); "DEFF" the gradients with respect to the effective parameters that the last
 * wn_train_bwd left (same layout; weight-normalised contexts after a wn_train_bwd, WN_E_STATE otherwise); "B1SUM" [L, G] dilated-conv bias +
 * conditioning bias; "SKIPB" [S] the scaled sum of the skip biases. */
int wn_debug_copy(wn_ctx* ctx, const char* name, int32_t layer, float* out, int64_t n, void* stream);
/* live HIP-event timing of the dominant training kernel (the gate GEMM, one launch per layer and step), recorded on the launch
 * stream between wn_profile(ctx,1) and wn_profile_result -- which SYNCHRONISES on the recorded events (bench only). */
int wn_profile(wn_ctx* ctx, int32_t enable);
int wn_profile_result(wn_ctx* ctx, double* total_ms, int64_t* launches);
/* the same launches by IN-KERNEL stamps (first workgroup's start .. last workgroup's end on the 100 MHz wall clock): the kernel's own
 * duration, as rocprofv3's kernel trace reports it -- without the wait behind the other stream's kernels the event bracket includes */
int wn_profile_kernel_result(wn_ctx* ctx, double* total_ms, int64_t* launches);
/* mean shader clock (MHz) INSIDE the same launches: workgroup 0 of each reads the shader-cycle counter and the 100 MHz wall clock at its start
 * and end.  The step runs at the chip's power limit (~1.35 kW), so the matrix peak that applies is 2500 TFLOP/s x clock / 2400 MHz. */
int wn_profile_kernel_clock(wn_ctx* ctx, double* mhz, int64_t* launches);
/* time rows (utterances x samples) one timed launch processed: the layer chain runs per half-batch on two streams */
int64_t wn_profile_rows_per_launch(const wn_ctx* ctx);
/* Device timeline of ONE training step from in-kernel stamps, no profiler attached (a profiler slows the host's enqueue enough to change
 * which stream runs ahead).  wn_trace_arm: every tile-engine and grouped weight-gradient launch of the `steps_from_now`-th next
 * wn_train_fwd .. wn_train_bwd stamps {first workgroup's start, last workgroup's end} on the 100 MHz wall clock into its own slot.
 * wn_trace_read (SYNCHRONISES the device): copies up to `cap` launches in enqueue order -- kind (0 gate, 1 out / skip / head conv,
 * 2 fp32-output GEMM, 3 d z, 4 head mask GEMM, 5 d x, 100 + n: grouped weight gradient with n A tiles), stream handle, start / end
 * ticks -- and returns their number (0 while no armed step has completed; negative wn_status on error). */
int wn_trace_arm(wn_ctx* ctx, int32_t steps_from_now);
int wn_trace_read(wn_ctx* ctx, int32_t cap, int32_t* kind, uint64_t* stream, uint64_t* start_ticks, uint64_t* end_ticks);
/* A/B switch of the stream structure.  0: default (2 when the batch has >= 2 utterances), 1: whole batch on the caller's stream,
 * 2: two half-batches on two streams */
int wn_set_batch_parts(wn_ctx* ctx, int32_t parts);
/* the dropout keep-mask of `layer` for the step seed, evaluated ON THE HOST by the very functions the kernels inline
 * (wn_layer_key / wn_drop_quad): out[i] = 1 if element first + i of the [rows][R] layer input is kept, else 0.  No context, no GPU:
 * pins the numpy mirror the parity tests hand to the oracle. */
int wn_test_dropout_mask(uint64_t seed, int32_t layer, float p, int64_t first, int64_t n, uint8_t* out);
/* wn_temper_noise evaluated ON THE HOST by the very function the noise kernels inline (csrc/wn_temper.h): in / out HOST float [rows, nps], in == out
 * allowed; mode 0 MoL (nps - 1 select entries, then the logistic draw), 1 Gaussian, 2 softmax.  No context, no GPU.  WN_E_ARG: a temperature outside [0, 2]
 * or not finite, nps < 1, a mode outside 0 ... 2, a null pointer. */
int wn_test_temper_noise(int32_t mode, int32_t nps, const float* in, float* out, int64_t rows, float tau_scale, float tau_select);
/* the fill of wn_synthesize(noise = NULL, seed) at a pair, alone: the device noise stream generated ALREADY TEMPERED into noise [T, B, noise_per_step]
 * (16-byte aligned).  Equal, bit for bit, to wn_fill_noise followed by wn_temper_noise; tools/temperature_timing.py times it. */
int wn_test_fill_noise_tempered(wn_ctx* ctx, float* noise, int32_t B, int32_t T, uint64_t seed, float tau_scale, float tau_select, void* stream);
/* which launches of this context take the 8-phase kernel (csrc/wn_tile8p.h; WN_GEMM8P in the environment of wn_create -- an A/B switch,
 * default 0): bit 0 = the gate GEMM, bit 1 = d x.  A model that does not fit the kernel reports 0 whatever the switch says. */
int wn_test_gemm8p_mask(const wn_ctx* ctx);
/* which launch kinds of this context issue v_mfma_f32_16x16x32_bf16 in the LDS-DMA ring kernel (csrc/wn_tile.h; WN_MFMA16 in the environment of
 * wn_create, unset: the library's default): bit 0 = the gate GEMM, bit 1 = d x, bit 2 = the other 32-channel-chunk launches (skip sum and full-tile
 * 1x1 convs, d z, the head's mask GEMMs).  Bits the library does not know are dropped. */
int wn_test_mfma16_mask(const wn_ctx* ctx);
/* The reuse contract of the training workspace: a step may assume NOTHING about bytes it did not write itself.  This hook fills every
 * buffer that only training steps write with 0xFF bytes -- a NaN in bf16 and in fp32 -- over its WHOLE allocation, not just the rows of the last step, by
 * hipMemsetAsync on `stream` (no kernel, no allocation), so that a launch which reads a row, a partial block or a tile it did not write this step shows in
 * its output (tests/test_hip_reuse.py).  Covered: the activation slabs X, XD, TS, U, R1, H2; the gradient slabs YHAT, DY, DPRE1, DSKIP, DZ, GX of every layer
 * (GX0 and GX1 are its first two), DC; the upsample levels CUP[], DCUP[] and cbt; the kept input copies XIN, CIN; the partial sums UPPART, the column-sum
 * partials and the split-K partials of the grouped weight gradients; the effective-gradient buffer ("DEFF"); the per-step global-conditioning tables (gate
 * bias per utterance, per-utterance column sums); every buffer the fp32 mode's state holds so far.  NOT touched: parameters, operand packs, the zero page,
 * "B1SUM", "SKIPB", the global-conditioning inputs of wn_set_global_condition, the device scalars and score partials, integer tables, profiling and trace
 * state, and all synthesis, stream and slot state.  The last forward is forgotten: wn_train_bwd is WN_E_STATE until the next wn_train_fwd.
 * The memsets are ordered on `stream` alone: pass the stream the last step was enqueued on (wn_train_fwd / wn_train_bwd join their own streams back into
 * it before they return), or synchronise the device first; work of that step which `stream` is not ordered after would race with the fill.
 * WN_E_ARG: ctx == NULL; WN_E_STATE: an inference-only context (it has no training workspace). */
int wn_test_poison_workspace(wn_ctx* ctx, void* stream);
/* The fragment-ordered bf16 operand packs that wn_pack_weights wrote.  kind: "w1", "wo", "ws", "w2T", "w1T" (one per layer) or "wskip", "wh1",
 * "wh2", "wh2T", "wh1T", "wcT" (`layer` ignored).  wn_test_pack_info: out = {M, K, kil, gate_interleave} (padded sizes; kil = 0 / 32 / 64 the
 * K interleave of the three taps).  wn_test_pack_copy: the M * K elements IN STORAGE ORDER, bf16 -> fp32, nothing un-shuffled, into the device
 * buffer out of n floats (SYNCHRONISES the device).  WN_E_ARG: unknown kind, layer outside [0, L), n < M * K, null pointer; WN_E_STATE: before
 * wn_pack_weights. */
int wn_test_pack_info(wn_ctx* ctx, const char* kind, int32_t layer, int32_t out[4]);
int wn_test_pack_copy(wn_ctx* ctx, const char* kind, int32_t layer, float* out, int64_t n);
/* the workgroup tables of the persistent synthesis pipeline for a model of L layers x P CUs per layer cut into ni instances (host logic only: no
 * context, no GPU): role[b] of workgroup b = layer << 8 | j, bit 23: a head (j = its index), bits 24-25: instance, -1: none; blk = the inverse
 * (ni = 1: [L * P + heads]; else ni x [L * P + 1]).  Block b runs on XCD b % 8: a layer's P CUs share an XCD, consecutive layers stay together.
 * Returns how many instances of the model the chip holds (1 ... 3), WN_E_SHAPE if ni do not fit. */
int wn_test_pipe_layout(int32_t L, int32_t P, int32_t ni, int32_t* role, int32_t cap_role, int32_t* blk, int32_t cap_blk, int32_t* grid, int32_t* heads);
/* device resources this PROCESS holds through the library (csrc/wn_dev.h; no context): out[0] live device / pinned buffers, [1] live streams,
 * [2] live events, [3] live graph execs, [4] buffer allocations ever.  Counts of the library's own handles: unlike hipMemGetInfo they do not move
 * with other processes on the device.  Take deltas around the life of a context: [0..3] return to where they were once it is destroyed. */
int wn_test_device_resources(int64_t out[5]);
/* device time of what a folded run adds around its span, by events on the caller's stream (tools/fold_timing.py): after wn_test_fold_timing(ctx, 1) every
 * wn_synthesize_folded records them; wn_test_fold_times SYNCHRONISES on the last run's and fills ms[0] the whole-utterance upsample (with the gather in front
 * of it), [1] the fold kernel, [2] the unfold kernel -- of the last group of equally long utterances when there are several.  WN_E_STATE without such a run. */
int wn_test_fold_timing(wn_ctx* ctx, int32_t enable);
int wn_test_fold_times(wn_ctx* ctx, double ms[3]);
/* the output stage's arithmetic on the host (no handle, no GPU): one row of n samples of cfg->in_type from y[-1] = carry_in, PCM scale pcm_scale as given
 * (cfg->gain is validated and not used).  out_f32 / out_pcm [n] and carry_out (y[n - 1]; carry_in for n = 0) are each optional.  WN_E_ARG as wn_post_create,
 * for in = NULL with n > 0, and for n < 0. */
int wn_test_post_host(const wn_post_config* cfg, const void* in, int64_t n, float carry_in, float pcm_scale, float* out_f32, int16_t* out_pcm, float* carry_out);
/* the reconstruction check on the host (no handle, no GPU): the arguments of a run with every pointer in HOST memory, evaluated by the very per-frame
 * and reduction functions the kernels inline (csrc/wn_melcmp.h), in the device's order: the same bits.  cfg->max_batch / max_frames of 0 here mean B and
 * the longest row.  Validates as a create followed by a run. */
int wn_test_melcmp_host(const wn_melcmp_config* cfg, const float* a, int32_t a_channels_first, int64_t a_pitch, const float* b, int32_t b_channels_first,
                        int64_t b_pitch, const int32_t* frames, int32_t B, float* per_frame, int64_t out_pitch, float* summary, int32_t* marks);
/* the training-summary statistics on the host (no handle, no GPU): the arguments of wn_stats_histogram / wn_stats_tensors with every pointer in HOST memory,
 * evaluated by the very element steps, cuts and joins the kernels inline (csrc/wn_stats.h), in the device's order: the same bits.  No max_rows / max_time /
 * max_tensors limit applies; otherwise validated as the device calls. */
int wn_test_stats_hist_host(const float* x, int64_t pitch, const int32_t* lengths, int32_t B, int32_t T, int64_t* bucket, double* summary);
int wn_test_stats_tensors_host(const float* flat, const int64_t* offsets, const int64_t* counts, int32_t nt, double* out);
/* the pitch check on the host (no handle, no GPU): the arguments of wn_pitch_run / wn_pitch_compare with every pointer in HOST memory, evaluated by the very
 * functions the kernels inline (csrc/wn_pitch.h), in the device's order: the same bits (the comparison's log2 in double is each side's library's).
 * Validated as a create followed by a run; the comparison hook has no max_batch / max_samples limit. */
int wn_test_pitch_host(const wn_pitch_config* cfg, const float* wav, int64_t ld, const int32_t* lengths, int32_t B, int32_t F_max, float* f0, float* ap, float* dprime);
int wn_test_pitch_compare_host(const float* f0_a, const float* f0_b, int64_t pitch, const int32_t* frames, int32_t B, float* table);
/* the spectral denoiser on the host (no handle, no GPU): fit and run in plain C++ float32 on HOST arrays, with the device's tables, packed spectrum and orders
 * of summation (csrc/wn_denoise.h); the matrix instruction's rounding inside a product is the device's own, so the two sides agree to float32 roundoff, not
 * bit for bit.  fit_wav != NULL: profile [1 + n_fft / 2] is fitted from fit_wav [fit_B, fit_ld] / fit_lengths and written; fit_wav == NULL: profile is read.
 * in != NULL: rows of in [B, in_pitch] -> out [B, out_pitch] at `strength` (in == out allowed, elements beyond lengths[b] untouched); in == NULL: fit only.
 * cfg->max_batch / max_samples are not limits here; otherwise validated as a create followed by the device calls. */
int wn_test_denoise_host(const wn_denoise_config* cfg, const float* fit_wav, int64_t fit_ld, const int32_t* fit_lengths, int32_t fit_B, float* profile,
                         const float* in, int64_t in_pitch, const int32_t* lengths, int32_t B, float strength, float* out, int64_t out_pitch);
/* the streaming denoiser on the host (no handle, no GPU): P pushes of B rows through the same state machine (counters, input tail, frame ring of R slots,
 * emit rule; csrc/wn_denoise_stream.h) in plain C++ float32 with the arithmetic of wn_test_denoise_host, so a row's concatenated output equals
 * wn_test_denoise_host of the whole row bit for bit.  Every pointer in HOST memory: in [P, B, in_pitch] elements of cfg->in_type, push p reads
 * n[p][b] of row b; out [P, B, out_pitch] receives n_out[p][b]; n, restart, final (either may be NULL), n_out: int32 [P, B].  profile [1 + n_fft / 2].
 * cfg->max_rows is not a limit here; otherwise validated as a create followed by the pushes (the first failing push ends the run with its code). */
int wn_test_denoise_stream_host(const wn_denoise_stream_config* cfg, const float* profile, float strength, const void* in, int64_t in_pitch, const int32_t* n,
                                const int32_t* restart, const int32_t* final, int32_t P, int32_t B, float* out, int64_t out_pitch, int32_t* n_out);
/* sample-rate conversion on the host (no handle, no GPU): P pushes of B rows through the state machine of wn_resample_push (counters, carried inputs, emit
 * rule; csrc/wn_resample.h) as a plain loop of fmaf -- the device's bits.  Every pointer in HOST memory: in [P, B, in_pitch] float, push p reads n[p][b] of
 * row b; out [P, B, out_pitch] receives n_out[p][b]; n, restart, final (either may be NULL), n_out: int32 [P, B].  A whole row is one push with final set.
 * cfg->max_rows is not a limit here and max_in = 0 means none; otherwise validated as a create followed by the pushes (the first failing push ends the run
 * with its code).  wn_test_resample_table: the float32 table C [L][T] of a configuration into table [cap]; WN_E_ARG when cap is below L x T. */
int wn_test_resample_host(const wn_resample_config* cfg, const float* in, int64_t in_pitch, const int32_t* n, const int32_t* restart, const int32_t* final, int32_t P,
                          int32_t B, float* out, int64_t out_pitch, int32_t* n_out);
int wn_test_resample_table(const wn_resample_config* cfg, float* table, int64_t cap);
/* the plan of wn_mel_stream_push (csrc/wn_mel_stream.h: validation, counters, the rule of readiness) over P pushes of B rows on a GEOMETRY-ONLY handle (WN_E_STATE
 * otherwise), on rows of its own and with no limit on B; no device, and `in` is only tested against NULL.  n, restart, final: HOST int32 [P, B] (restart and final may be
 * NULL).  Per push: status [P] is what the push would return (a refused push changes no row); per push and row, [P, B]: n_out, first_frame (the index of the row's first
 * new frame), and after the push tail_len (carried samples; always below win_size), S and F. */
int wn_test_mel_stream_plan(const wn_mel_stream* h, const float* in, int64_t in_pitch, const int32_t* n, const int32_t* restart, const int32_t* final, int32_t P, int32_t B,
                            int64_t out_pitch, int32_t* status, int32_t* n_out, int64_t* first_frame, int32_t* tail_len, int64_t* S, int64_t* F);
/* Griffin-Lim test hooks.  wn_test_griffin_store_spectrum: with on != 0 the iterations of later runs take the variant of the tile kernel that also stores
 * the spectrum BEFORE the projection (the last iteration's survives) to a workspace reserved by this call; the result of a run is the same bits either way.
 * wn_test_griffin_copy (SYNCHRONISES the stream): what = 0 the magnitudes of the last run into dst HOST float [B, F_max, 1 + n_fft / 2], what = 1 that
 * spectrum into dst HOST float [B, F_max, 1 + n_fft / 2, 2] (re, im); frames beyond a row's are left alone.
 * wn_test_griffin_host: a run on the host (no handle, no GPU), every pointer in HOST memory, in plain C++ float32 with the device's tables, packed
 * spectrum and orders of summation (csrc/wn_griffin.h); the two sides agree to float32 roundoff, not bit for bit.  mag_out [B, F_max, 1 + n_fft / 2] and
 * pre_out [B, F_max, 1 + n_fft / 2, 2] (the spectrum before the last projection) are optional.  cfg->max_batch / max_frames are not limits here. */
int wn_test_griffin_store_spectrum(wn_griffin* h, int32_t on);
int wn_test_griffin_copy(wn_griffin* h, int32_t what, float* dst, int32_t F_max, void* stream);
int wn_test_griffin_host(const wn_griffin_config* cfg, const float* pinv, const float* src, int32_t src_kind, int32_t F_max, const int32_t* frames, int32_t B,
                         const float* u, const float* y0, int64_t y0_pitch, int32_t iters, float* out, int64_t out_pitch, float* mag_out, float* pre_out);
/* fp32 training mode (csrc/wn_f32.hip), ONE launch on operands the caller owns (device pointers; tests/test_hip_f32_kernels.py).  Each goes through the very
 * function the chain calls, so the grid computation, the partial-sum capacity check and the slab reduction are under test.  Rows are b * T + t for B utterances
 * of T samples; the context's forward shape and dropout seed are set for the call and restored after it.  WN_E_STATE: not an fp32-mode training context;
 * WN_E_ARG: B > max_batch, T > max_time, a null operand.
 * wn_test_f32_sgemm: Out[row][m] (out_bot: Out[b][m][t]) = mask(relu(((accumulate ? Out : 0) + drop_out(alpha * sum_k drop_a(In[row + shift][col0 + k]) *
 *   W[k * wk + m * wm]) + bias[b * bias_bstride + m] + add[row][m]) * scale)); a row with t + shift outside [0, T) of ITS utterance contributes zero.  thresh16 > 0:
 *   dropout from (key_lo, key_hi) on element row * drop_ld + column of the A operand, or of the output with drop_on_out.  mask, bias, add may be NULL.
 * wn_test_f32_wgrad: out[k][m] (row pitch ldo) = alpha * sum_rows drop(A[row + shift][k]) * Bm[row][m]; bias_out / bias_out2 (either may be NULL) = alpha * column
 *   sums of Bm.  A == NULL: only the column sums.  drop_layer >= 0: the context's dropout with the key of (seed, drop_layer) on element row * lda + k of A.
 *   WN_E_STATE when B * ceil(T / 2048) * (K + 1) * M exceeds the context's partial-sum buffer.
 * wn_test_f32_gate: U [rows][GH] = tanh(Z_a) * sigmoid(Z_b) of Z [rows][2 GH]; DZ [rows][2 GH] = the gate's derivative times GU [rows][GH]. */
int wn_test_f32_sgemm(wn_ctx* ctx, int32_t B, int32_t T, const float* In, int32_t ld_in, int32_t col0, int32_t shift, const float* W, int32_t wk, int32_t wm,
                      int32_t K, int32_t M, float* Out, int32_t ld_out, int32_t accumulate, const float* mask, int32_t ld_mask, int32_t drop_on_out,
                      float alpha, float scale, const float* bias, int32_t bias_bstride, const float* add, int32_t ld_add, int32_t relu, int32_t out_bot,
                      uint32_t key_lo, uint32_t key_hi, uint32_t thresh16, float keep_scale, int32_t drop_ld, void* stream);
int wn_test_f32_wgrad(wn_ctx* ctx, int32_t B, int32_t T, const float* A, int32_t lda, int32_t shift, int32_t K, const float* Bm, int32_t ldb, int32_t M,
                      float* out, int32_t ldo, float alpha, int32_t drop_layer, uint64_t seed, float* bias_out, float* bias_out2, void* stream);
int wn_test_f32_gate(wn_ctx* ctx, const float* Z, const float* GU, float* U, float* DZ, int64_t rows, int32_t GH, void* stream);
/* Alignment check test hooks.  wn_test_align_host: a run on the host (no handle, no GPU), every pointer in HOST memory, evaluated by the very functions
 * the kernels inline (csrc/wn_align.h): the same bits.  cfg->max_batch / max_frames_* are not limits here; otherwise validated as a create followed by a
 * run.  The stages are optional outputs with Fa_max / Fb_max the longest rows of the call: cep_a [B, Fa_max, n_cep], cep_b [B, Fb_max, n_cep], cost and dm
 * [B, Fa_max, Fb_max]; cells beyond a row's extent are left alone.
 * wn_test_align_dp_host: recurrence, back-trace and outputs on a caller's HOST cost matrix [B, Fa_max, Fb_max] instead of mels, band as given; dm optional.
 * wn_test_align_dp: the same on the device through the kernels of wn_align_run, cost a DEVICE float [B, Fa_max, Fb_max]; validated as a run.
 * wn_test_align_store_matrix: with on != 0 later runs also keep Dm in a buffer [max_batch, max_frames_a, max_frames_b] reserved by this call; the results
 * of a run are the same bits either way.  wn_test_align_copy (SYNCHRONISES the stream): the handle's own scratch of the last run into dst HOST float [cap],
 * what = 0 the cepstra of a [max_batch, max_frames_a, n_cep], 1 of b [max_batch, max_frames_b, n_cep], 2 the cost matrix and 3 Dm [max_batch, max_frames_a,
 * max_frames_b]; WN_E_ARG when cap is below that size, WN_E_STATE for Dm before wn_test_align_store_matrix. */
int wn_test_align_host(const wn_align_config* cfg, const float* a, int32_t a_channels_first, int64_t a_pitch, const float* b, int32_t b_channels_first, int64_t b_pitch,
                       const int32_t* frames_a, const int32_t* frames_b, int32_t B, int32_t* path, int64_t path_pitch, int32_t* map_ab, int64_t map_a_pitch,
                       int32_t* map_ba, int64_t map_b_pitch, float* summary, float* cep_a, float* cep_b, float* cost, float* dm);
int wn_test_align_dp_host(int32_t band, const float* cost, int32_t Fa_max, int32_t Fb_max, const int32_t* frames_a, const int32_t* frames_b, int32_t B, int32_t* path,
                          int64_t path_pitch, int32_t* map_ab, int64_t map_a_pitch, int32_t* map_ba, int64_t map_b_pitch, float* summary, float* dm);
int wn_test_align_dp(wn_align* h, const float* cost, int32_t Fa_max, int32_t Fb_max, const int32_t* frames_a, const int32_t* frames_b, int32_t B, int32_t* path,
                     int64_t path_pitch, int32_t* map_ab, int64_t map_a_pitch, int32_t* map_ba, int64_t map_b_pitch, float* summary, void* stream);
int wn_test_align_store_matrix(wn_align* h, int32_t on);
int wn_test_align_copy(wn_align* h, int32_t what, float* dst, int64_t cap, void* stream);
#endif /* WN_NO_TEST_HOOKS */

#ifdef __cplusplus
}
#endif
#endif /* WAVENET_MI355_H */
