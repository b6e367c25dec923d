"""ctypes binding of libwavenet_mi355.so (C ABI: include/wavenet_mi355.h).

This is the ONLY compute path of the package: there is no CPU / eager fallback.  If the shared
library has not been built (``python tacotron-2_amd/csrc/build.py``) importing the engine raises.
PyTorch is used for device memory, streams and torch.distributed only.
"""
import ctypes
import os
from collections import OrderedDict

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.normpath(os.path.join(_HERE, '..', '..', 'csrc', 'libwavenet_mi355.so'))
# test / tool hook: another build of the library -- the ASAN / UBSAN build of the host side (csrc/build.py --sanitize), a diagnostic build
# (--ablate, --pipe-svc) or an earlier build for an A/B; never set by the product
if os.environ.get('WN_MI355_TEST_LIB'):
    LIB_PATH = os.environ['WN_MI355_TEST_LIB']

WN_ABI_VERSION = 4
WN_MAX_UPSAMPLE = 8
INPUT_TYPES = {'raw': 0, 'mulaw': 1, 'mulaw-quantize': 2}
UPSAMPLE_TYPES = {'NearestNeighbor': 0, '2D': 1, 'SubPixel': 2, '1D': 3, 'Resize': 4}
ACTIVATIONS = {None: 0, 'None': 0, 'Relu': 1, 'LeakyRelu': 2}
LR_SCHEDULES = {'exponential': 0, 'noam': 1}
COMPUTE_DTYPES = {'bf16': 0, 'fp32': 1, 'float32': 1}      # wn_compute_dtype: 'fp32' = the reference's arithmetic for forward, loss and backward (csrc/wn_f32.hip)
STATUS = {0: 'WN_OK', -1: 'WN_E_ARG', -2: 'WN_E_SHAPE', -3: 'WN_E_HIP', -4: 'WN_E_UNSUPPORTED', -5: 'WN_E_STATE'}


class WnConfig(ctypes.Structure):
    _fields_ = [
        ('abi_version', ctypes.c_int32),
        ('layers', ctypes.c_int32), ('stacks', ctypes.c_int32),
        ('residual_channels', ctypes.c_int32), ('gate_channels', ctypes.c_int32),
        ('skip_out_channels', ctypes.c_int32), ('out_channels', ctypes.c_int32),
        ('kernel_size', ctypes.c_int32), ('cin_channels', ctypes.c_int32),
        ('input_type', ctypes.c_int32), ('quantize_channels', ctypes.c_int32),
        ('use_bias', ctypes.c_int32), ('legacy', ctypes.c_int32), ('residual_legacy', ctypes.c_int32),
        ('log_scale_min', ctypes.c_float), ('log_scale_min_gauss', ctypes.c_float),
        ('cdf_loss', ctypes.c_int32),
        ('upsample_type', ctypes.c_int32), ('upsample_activation', ctypes.c_int32),
        ('n_upsample', ctypes.c_int32), ('upsample_scales', ctypes.c_int32 * WN_MAX_UPSAMPLE),
        ('freq_axis_kernel_size', ctypes.c_int32), ('leaky_alpha', ctypes.c_float),
        ('dropout', ctypes.c_float), ('clip_gradients', ctypes.c_int32),
        ('gradient_max_norm', ctypes.c_float), ('gradient_max_value', ctypes.c_float),
        ('adam_beta1', ctypes.c_float), ('adam_beta2', ctypes.c_float),
        ('adam_epsilon', ctypes.c_float), ('ema_decay', ctypes.c_float),
        ('max_batch', ctypes.c_int32), ('max_time', ctypes.c_int32),
        ('gin_channels', ctypes.c_int32), ('use_speaker_embedding', ctypes.c_int32), ('n_speakers', ctypes.c_int32),
        ('weight_normalization', ctypes.c_int32),
        ('inference_only', ctypes.c_int32),
        ('grad_buckets', ctypes.c_int32),
        ('compute_dtype', ctypes.c_int32),
    ]


class WnMelConfig(ctypes.Structure):
    _fields_ = [
        ('abi_version', ctypes.c_int32), ('sample_rate', ctypes.c_int32),
        ('n_fft', ctypes.c_int32), ('hop_size', ctypes.c_int32), ('win_size', ctypes.c_int32), ('num_mels', ctypes.c_int32),
        ('magnitude_power', ctypes.c_float), ('min_level_db', ctypes.c_float), ('ref_level_db', ctypes.c_float),
        ('max_abs_value', ctypes.c_float), ('preemphasis', ctypes.c_float),
        ('signal_normalization', ctypes.c_int32), ('allow_clipping', ctypes.c_int32), ('symmetric_mels', ctypes.c_int32),
        ('max_batch', ctypes.c_int32), ('max_samples', ctypes.c_int64),
    ]


class WnPostConfig(ctypes.Structure):
    _fields_ = [('abi_version', ctypes.c_int32), ('max_rows', ctypes.c_int32), ('in_type', ctypes.c_int32), ('deemphasis', ctypes.c_float), ('gain', ctypes.c_float)]


class WnMelcmpConfig(ctypes.Structure):
    _fields_ = [('abi_version', ctypes.c_int32), ('num_mels', ctypes.c_int32), ('n_cep', ctypes.c_int32), ('unit_db', ctypes.c_float), ('alarm_db', ctypes.c_float),
                ('max_batch', ctypes.c_int32), ('max_frames', ctypes.c_int32)]


class WnAlignConfig(ctypes.Structure):
    _fields_ = [('abi_version', ctypes.c_int32), ('num_mels', ctypes.c_int32), ('n_cep', ctypes.c_int32), ('unit_db', ctypes.c_float), ('band', ctypes.c_int32),
                ('max_batch', ctypes.c_int32), ('max_frames_a', ctypes.c_int32), ('max_frames_b', ctypes.c_int32)]


class WnStatsConfig(ctypes.Structure):
    _fields_ = [('abi_version', ctypes.c_int32), ('max_rows', ctypes.c_int32), ('max_time', ctypes.c_int32), ('max_tensors', ctypes.c_int32)]


class WnPitchConfig(ctypes.Structure):
    _fields_ = [('abi_version', ctypes.c_int32), ('sample_rate', ctypes.c_int32), ('hop', ctypes.c_int32), ('window', ctypes.c_int32), ('tau_min', ctypes.c_int32),
                ('tau_max', ctypes.c_int32), ('threshold', ctypes.c_float), ('max_batch', ctypes.c_int32), ('max_samples', ctypes.c_int64)]


class WnDenoiseConfig(ctypes.Structure):
    _fields_ = [('abi_version', ctypes.c_int32), ('n_fft', ctypes.c_int32), ('hop', ctypes.c_int32), ('max_batch', ctypes.c_int32), ('max_samples', ctypes.c_int64)]


class WnDenoiseStreamConfig(ctypes.Structure):
    _fields_ = [('abi_version', ctypes.c_int32), ('n_fft', ctypes.c_int32), ('hop', ctypes.c_int32), ('max_rows', ctypes.c_int32), ('max_push', ctypes.c_int32),
                ('in_type', ctypes.c_int32)]


class WnGriffinConfig(ctypes.Structure):
    _fields_ = [('abi_version', ctypes.c_int32), ('n_fft', ctypes.c_int32), ('win_size', ctypes.c_int32), ('hop', ctypes.c_int32), ('num_mels', ctypes.c_int32),
                ('magnitude_power', ctypes.c_float), ('power', ctypes.c_float), ('min_level_db', ctypes.c_float), ('ref_level_db', ctypes.c_float),
                ('max_abs_value', ctypes.c_float), ('signal_normalization', ctypes.c_int32), ('allow_clipping', ctypes.c_int32), ('symmetric_mels', ctypes.c_int32),
                ('max_batch', ctypes.c_int32), ('max_frames', ctypes.c_int32)]


class WnResampleConfig(ctypes.Structure):
    _fields_ = [('abi_version', ctypes.c_int32), ('max_rows', ctypes.c_int32), ('max_in', ctypes.c_int32), ('sr_in', ctypes.c_int32), ('sr_out', ctypes.c_int32),
                ('zeros', ctypes.c_int32), ('beta', ctypes.c_double), ('rolloff', ctypes.c_double)]


class WnFoldRow(ctypes.Structure):
    """wn_fold_row: one row of a folded run, in mel frames of utterance `utt`."""
    _fields_ = [('utt', ctypes.c_int32), ('first', ctypes.c_int32), ('frames', ctypes.c_int32), ('keep', ctypes.c_int32), ('fade', ctypes.c_int32)]


FADE_KINDS = {'equal_power': 0, 'linear': 1}


class WnError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__('%s: %s' % (STATUS.get(code, code), msg))
        self.code = code


_lib = None


def load_library():
    """dlopen the HIP library; raises (loudly) if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError('libwavenet_mi355.so not found at %s -- the HIP extension is the only compute '
                           'path of this package; build it with `python tacotron-2_amd/csrc/build.py`' % LIB_PATH)
    # PyTorch-ROCm bundles its own libamdhip64: it must be the HIP runtime of the process (device memory and streams come from
    # torch), so import torch BEFORE the library is dlopen'ed -- loaded the other way round, /opt/rocm's runtime is mapped first
    # and the second runtime finds "no ROCm-capable device".
    import torch  # noqa: F401
    lib = ctypes.CDLL(LIB_PATH)
    vp, i32, i64, f32, u64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_uint64
    sigs = {
        'wn_create': (ctypes.c_int, [ctypes.POINTER(WnConfig), ctypes.POINTER(vp)]),
        'wn_destroy': (None, [vp]),
        'wn_last_error': (ctypes.c_char_p, [vp]),
        'wn_receptive_field': (ctypes.c_int, [vp]),
        'wn_param_count': (i64, [vp]),
        'wn_num_tensors': (ctypes.c_int, [vp]),
        'wn_tensor_info': (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_char_p, ctypes.POINTER(i32), ctypes.POINTER(i32), ctypes.POINTER(i64)]),
        'wn_pack_weights': (ctypes.c_int, [vp, vp, vp]),
        'wn_train_fwd': (ctypes.c_int, [vp, vp, vp, vp, vp, i32, i32, i32, u64, vp, vp, vp]),
        'wn_train_bwd': (ctypes.c_int, [vp, vp, vp]),
        'wn_bwd_num_buckets': (ctypes.c_int, [vp]),
        'wn_bwd_bucket_range': (ctypes.c_int, [vp, i32, ctypes.POINTER(i64), ctypes.POINTER(i64)]),
        'wn_bwd_wait_bucket': (ctypes.c_int, [vp, i32, vp]),
        'wn_get_upsampled_features': (ctypes.c_int, [vp, vp, vp]),
        'wn_optim_step': (ctypes.c_int, [vp, vp, vp, vp, vp, vp, f32, i64, vp]),
        'wn_learning_rate': (f32, [i32, f32, i64, f32, i64, f32]),
        'wn_synthesize': (ctypes.c_int, [vp, vp, i32, i32, vp, u64, vp, vp, vp, i32, vp]),
        'wn_synthesize_wide': (ctypes.c_int, [vp, vp, i32, i32, vp, u64, vp, vp, vp, i32, vp]),
        'wn_noise_per_step': (ctypes.c_int, [vp]),
        'wn_fill_noise': (ctypes.c_int, [vp, vp, i32, i32, u64, vp]),
        'wn_synth_set_temperature': (ctypes.c_int, [vp, f32, f32]),
        'wn_synth_get_temperature': (ctypes.c_int, [vp, ctypes.POINTER(f32), ctypes.POINTER(f32)]),
        'wn_synth_set_slot_temperature': (ctypes.c_int, [vp, i32, f32, f32]),
        'wn_temper_noise': (ctypes.c_int, [vp, vp, vp, i32, i32, f32, f32, vp]),
        'wn_test_temper_noise': (ctypes.c_int, [i32, i32, vp, vp, i64, f32, f32]),
        'wn_test_fill_noise_tempered': (ctypes.c_int, [vp, vp, i32, i32, u64, f32, f32, vp]),
        'wn_synth_check': (ctypes.c_int, [vp]),
        'wn_synth_last_path': (ctypes.c_int, [vp]),
        'wn_test_gemm8p_mask': (ctypes.c_int, [vp]),
        'wn_test_mfma16_mask': (ctypes.c_int, [vp]),
        'wn_test_poison_workspace': (ctypes.c_int, [vp, vp]),
        'wn_test_pack_info': (ctypes.c_int, [vp, ctypes.c_char_p, i32, ctypes.POINTER(i32)]),
        'wn_test_pack_copy': (ctypes.c_int, [vp, ctypes.c_char_p, i32, vp, i64]),
        'wn_test_f32_sgemm': (ctypes.c_int, [vp, i32, i32, vp, i32, i32, i32, vp, i32, i32, i32, i32, vp, i32, i32, vp, i32, i32, f32, f32, vp, i32, vp, i32, i32, i32,
                                             ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, f32, i32, vp]),
        'wn_test_f32_wgrad': (ctypes.c_int, [vp, i32, i32, vp, i32, i32, i32, vp, i32, i32, vp, i32, f32, i32, u64, vp, vp, vp]),
        'wn_test_f32_gate': (ctypes.c_int, [vp, vp, vp, vp, vp, i64, i32, vp]),
        'wn_test_pipe_layout': (ctypes.c_int, [i32, i32, i32, vp, i32, vp, i32, vp, vp]),
        'wn_test_device_resources': (ctypes.c_int, [ctypes.POINTER(i64)]),
        'wn_synth_pipe_dtype': (ctypes.c_int, [vp, i32]),
        'wn_synth_last_instances': (ctypes.c_int, [vp]),
        'wn_synth_last_config': (ctypes.c_int, [vp, ctypes.POINTER(i32), i32]),
        'wn_synth_last_batched': (ctypes.c_int, [vp]),
        'wn_synth_pipe_eligible': (ctypes.c_int, [vp, i32]),
        'wn_synth_stream_lookahead': (ctypes.c_int, [ctypes.POINTER(WnConfig), ctypes.POINTER(i32), ctypes.POINTER(i32)]),
        'wn_synth_stream_begin': (ctypes.c_int, [vp, i32, u64, i32, vp]),
        'wn_synth_stream_push': (ctypes.c_int, [vp, vp, i32, i32, vp, vp, vp, vp, ctypes.POINTER(i32), vp]),
        'wn_synth_stream_end': (ctypes.c_int, [vp]),
        'wn_synth_slots_begin': (ctypes.c_int, [vp, i32, i32, vp]),
        'wn_synth_wide_slots_begin': (ctypes.c_int, [vp, i32, i32, vp]),
        'wn_synth_slot_open': (ctypes.c_int, [vp, i32, u64, vp, vp]),
        'wn_synth_slots_push': (ctypes.c_int, [vp, vp, i32, ctypes.POINTER(i32), ctypes.POINTER(i32), vp, vp, vp, vp, i32, ctypes.POINTER(i32), vp]),
        'wn_synth_slot_abandon': (ctypes.c_int, [vp, i32]),
        'wn_synth_slot_frames_done': (ctypes.c_int, [vp, i32]),
        'wn_synth_slots_end': (ctypes.c_int, [vp]),
        'wn_fold_plan': (ctypes.c_int, [ctypes.POINTER(i32), i32, i32, i32, i32, i32, ctypes.POINTER(WnFoldRow), i32]),
        'wn_fold_check': (ctypes.c_int, [ctypes.POINTER(i32), i32, ctypes.POINTER(WnFoldRow), i32, ctypes.c_char_p, i32]),
        'wn_fold_weights': (ctypes.c_int, [i32, i32, vp, vp]),
        'wn_synthesize_folded': (ctypes.c_int, [vp, vp, ctypes.POINTER(i32), i32, ctypes.POINTER(WnFoldRow), i32, i32, vp, vp, u64, vp, vp, i32, vp, vp, i32, i32, vp]),
        'wn_test_fold_timing': (ctypes.c_int, [vp, i32]),
        'wn_test_fold_times': (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_double)]),
        'wn_sample': (ctypes.c_int, [vp, vp, i32, i32, vp, vp, vp]),
        'wn_mulaw': (ctypes.c_int, [vp, vp, i64, vp]),
        'wn_inv_mulaw': (ctypes.c_int, [vp, vp, i64, vp]),
        'wn_mulaw_quantize': (ctypes.c_int, [vp, vp, i64, vp]),
        'wn_inv_mulaw_quantize': (ctypes.c_int, [vp, vp, i64, vp]),
        'wn_argmax_channels': (ctypes.c_int, [vp, vp, i32, i32, i32, vp]),
        'wn_loss': (ctypes.c_int, [vp, vp, vp, vp, i32, i32, i32, vp, vp]),
        'wn_eval_fwd': (ctypes.c_int, [vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp]),
        'wn_score': (ctypes.c_int, [vp, vp, vp, vp, i32, i32, i32, vp, vp, vp]),
        'wn_profile': (ctypes.c_int, [vp, i32]),
        'wn_profile_result': (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(i64)]),
        'wn_profile_kernel_result': (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(i64)]),
        'wn_profile_kernel_clock': (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(i64)]),
        'wn_profile_rows_per_launch': (i64, [vp]),
        'wn_set_batch_parts': (ctypes.c_int, [vp, i32]),
        'wn_debug_copy': (ctypes.c_int, [vp, ctypes.c_char_p, i32, vp, i64, vp]),
        'wn_trace_arm': (ctypes.c_int, [vp, i32]),
        'wn_trace_read': (ctypes.c_int, [vp, i32, ctypes.POINTER(i32), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
        'wn_set_global_condition': (ctypes.c_int, [vp, vp, i32, vp]),
        'wn_workspace_bytes': (i64, [vp]),
        'wn_dominant_kernel_name': (ctypes.c_char_p, []),
        'wn_test_dropout_mask': (ctypes.c_int, [ctypes.c_uint64, i32, ctypes.c_float, i64, i64, vp]),
        'wn_mel_create': (ctypes.c_int, [ctypes.POINTER(WnMelConfig), vp, ctypes.POINTER(vp)]),
        'wn_mel_destroy': (None, [vp]),
        'wn_mel_last_error': (ctypes.c_char_p, [vp]),
        'wn_mel_num_frames': (i64, [vp, i64]),
        'wn_mel_frame_tile': (ctypes.c_int, [vp]),
        'wn_mel_peak': (ctypes.c_int, [vp, vp, i64, ctypes.POINTER(i32), i32, vp, vp]),
        'wn_mel_run': (ctypes.c_int, [vp, vp, i64, ctypes.POINTER(i32), vp, vp, i32, i32, i32, vp]),
        'wn_post_create': (ctypes.c_int, [ctypes.POINTER(WnPostConfig), ctypes.POINTER(vp)]),
        'wn_post_destroy': (None, [vp]),
        'wn_post_last_error': (ctypes.c_char_p, [vp]),
        'wn_post_push': (ctypes.c_int, [vp, vp, i64, ctypes.POINTER(i32), ctypes.POINTER(i32), i32, vp, vp, i64, vp, vp]),
        'wn_post_finish': (ctypes.c_int, [vp, vp, i64, ctypes.POINTER(i32), i32, vp, vp, i64, vp, vp]),
        'wn_test_post_host': (ctypes.c_int, [ctypes.POINTER(WnPostConfig), vp, i64, f32, f32, vp, vp, ctypes.POINTER(f32)]),
        'wn_melcmp_create': (ctypes.c_int, [ctypes.POINTER(WnMelcmpConfig), ctypes.POINTER(vp)]),
        'wn_melcmp_destroy': (None, [vp]),
        'wn_melcmp_last_error': (ctypes.c_char_p, [vp]),
        'wn_melcmp_run': (ctypes.c_int, [vp, vp, i32, i64, vp, i32, i64, ctypes.POINTER(i32), i32, vp, i64, vp, vp, vp]),
        'wn_test_melcmp_host': (ctypes.c_int, [ctypes.POINTER(WnMelcmpConfig), vp, i32, i64, vp, i32, i64, ctypes.POINTER(i32), i32, vp, i64, vp, vp]),
        'wn_stats_create': (ctypes.c_int, [ctypes.POINTER(WnStatsConfig), ctypes.POINTER(vp)]),
        'wn_stats_destroy': (None, [vp]),
        'wn_stats_last_error': (ctypes.c_char_p, [vp]),
        'wn_stats_hist_limits': (ctypes.c_int, [vp, i32]),
        'wn_stats_histogram': (ctypes.c_int, [vp, vp, i64, vp, i32, i32, vp, vp, vp]),
        'wn_stats_set_tensors': (ctypes.c_int, [vp, vp, vp, i32]),
        'wn_stats_tensors': (ctypes.c_int, [vp, vp, vp, vp]),
        'wn_test_stats_hist_host': (ctypes.c_int, [vp, i64, vp, i32, i32, vp, vp]),
        'wn_test_stats_tensors_host': (ctypes.c_int, [vp, vp, vp, i32, vp]),
        'wn_pitch_create': (ctypes.c_int, [ctypes.POINTER(WnPitchConfig), ctypes.POINTER(vp)]),
        'wn_pitch_destroy': (None, [vp]),
        'wn_pitch_last_error': (ctypes.c_char_p, [vp]),
        'wn_pitch_num_frames': (i64, [vp, i64]),
        'wn_pitch_frame_tile': (ctypes.c_int, [vp]),
        'wn_pitch_run': (ctypes.c_int, [vp, vp, i64, ctypes.POINTER(i32), i32, i32, vp, vp, vp, vp]),
        'wn_pitch_compare': (ctypes.c_int, [vp, vp, vp, i64, ctypes.POINTER(i32), i32, vp, vp]),
        'wn_test_pitch_host': (ctypes.c_int, [ctypes.POINTER(WnPitchConfig), vp, i64, ctypes.POINTER(i32), i32, i32, vp, vp, vp]),
        'wn_test_pitch_compare_host': (ctypes.c_int, [vp, vp, i64, ctypes.POINTER(i32), i32, vp]),
        'wn_denoise_create': (ctypes.c_int, [ctypes.POINTER(WnDenoiseConfig), ctypes.POINTER(vp)]),
        'wn_denoise_destroy': (None, [vp]),
        'wn_denoise_last_error': (ctypes.c_char_p, [vp]),
        'wn_denoise_num_frames': (i64, [vp, i64]),
        'wn_denoise_fit': (ctypes.c_int, [vp, vp, i64, ctypes.POINTER(i32), i32, vp]),
        'wn_denoise_set_profile': (ctypes.c_int, [vp, vp, vp]),
        'wn_denoise_get_profile': (ctypes.c_int, [vp, vp, vp]),
        'wn_denoise_run': (ctypes.c_int, [vp, vp, i64, ctypes.POINTER(i32), i32, f32, vp, i64, vp]),
        'wn_test_denoise_host': (ctypes.c_int, [ctypes.POINTER(WnDenoiseConfig), vp, i64, ctypes.POINTER(i32), i32, vp, vp, i64, ctypes.POINTER(i32), i32, f32, vp, i64]),
        'wn_denoise_stream_create': (ctypes.c_int, [ctypes.POINTER(WnDenoiseStreamConfig), ctypes.POINTER(vp)]),
        'wn_denoise_stream_destroy': (None, [vp]),
        'wn_denoise_stream_last_error': (ctypes.c_char_p, [vp]),
        'wn_denoise_stream_set_profile': (ctypes.c_int, [vp, vp, vp]),
        'wn_denoise_stream_take_profile': (ctypes.c_int, [vp, vp, vp]),
        'wn_denoise_stream_ready': (i64, [vp, i64, i32]),
        'wn_denoise_stream_push': (ctypes.c_int, [vp, vp, i64, ctypes.POINTER(i32), ctypes.POINTER(i32), ctypes.POINTER(i32), i32, f32, vp, i64, ctypes.POINTER(i32), vp]),
        'wn_test_denoise_stream_host': (ctypes.c_int, [ctypes.POINTER(WnDenoiseStreamConfig), vp, f32, vp, i64, vp, vp, vp, i32, i32, vp, i64, vp]),
        'wn_resample_create': (ctypes.c_int, [ctypes.POINTER(WnResampleConfig), ctypes.POINTER(vp)]),
        'wn_resample_destroy': (None, [vp]),
        'wn_resample_last_error': (ctypes.c_char_p, [vp]),
        'wn_resample_num_out': (i64, [vp, i64]),
        'wn_resample_ready': (i64, [vp, i64, i32]),
        'wn_resample_taps': (ctypes.c_int, [vp, ctypes.POINTER(i32), ctypes.POINTER(i32), ctypes.POINTER(i32)]),
        'wn_resample_run': (ctypes.c_int, [vp, vp, i64, ctypes.POINTER(i32), i32, vp, i64, vp]),
        'wn_resample_push': (ctypes.c_int, [vp, vp, i64, ctypes.POINTER(i32), ctypes.POINTER(i32), ctypes.POINTER(i32), i32, vp, i64, ctypes.POINTER(i32), vp]),
        'wn_test_resample_host': (ctypes.c_int, [ctypes.POINTER(WnResampleConfig), vp, i64, vp, vp, vp, i32, i32, vp, i64, vp]),
        'wn_test_resample_table': (ctypes.c_int, [ctypes.POINTER(WnResampleConfig), vp, i64]),
        'wn_mel_stream_create': (ctypes.c_int, [ctypes.POINTER(WnMelConfig), vp, i32, i32, ctypes.POINTER(vp)]),
        'wn_mel_stream_destroy': (None, [vp]),
        'wn_mel_stream_last_error': (ctypes.c_char_p, [vp]),
        'wn_mel_stream_ready': (i64, [vp, i64, i32]),
        'wn_mel_stream_push': (ctypes.c_int, [vp, vp, i64, ctypes.POINTER(i32), ctypes.POINTER(i32), ctypes.POINTER(i32), ctypes.POINTER(f32), i32, vp, i64, i32, ctypes.POINTER(i32), vp]),
        'wn_test_mel_stream_plan': (ctypes.c_int, [vp, vp, i64, vp, vp, vp, i32, i32, i64, vp, vp, vp, vp, vp, vp]),
        'wn_griffin_create': (ctypes.c_int, [ctypes.POINTER(WnGriffinConfig), vp, ctypes.POINTER(vp)]),
        'wn_griffin_destroy': (None, [vp]),
        'wn_griffin_last_error': (ctypes.c_char_p, [vp]),
        'wn_griffin_num_samples': (i64, [vp, i64]),
        'wn_griffin_run': (ctypes.c_int, [vp, vp, i32, i32, ctypes.POINTER(i32), i32, vp, vp, i64, i32, i32, vp, i64, vp]),
        'wn_test_griffin_store_spectrum': (ctypes.c_int, [vp, i32]),
        'wn_test_griffin_copy': (ctypes.c_int, [vp, i32, vp, i32, vp]),
        'wn_test_griffin_host': (ctypes.c_int, [ctypes.POINTER(WnGriffinConfig), vp, vp, i32, i32, ctypes.POINTER(i32), i32, vp, vp, i64, i32, vp, i64, vp, vp]),
        'wn_align_create': (ctypes.c_int, [ctypes.POINTER(WnAlignConfig), ctypes.POINTER(vp)]),
        'wn_align_destroy': (None, [vp]),
        'wn_align_last_error': (ctypes.c_char_p, [vp]),
        'wn_align_tile': (ctypes.c_int, [vp]),
        'wn_align_run': (ctypes.c_int, [vp, vp, i32, i64, vp, i32, i64, ctypes.POINTER(i32), ctypes.POINTER(i32), i32, vp, i64, vp, i64, vp, i64, vp, vp]),
        'wn_test_align_host': (ctypes.c_int, [ctypes.POINTER(WnAlignConfig), vp, i32, i64, vp, i32, i64, ctypes.POINTER(i32), ctypes.POINTER(i32), i32, vp, i64, vp, i64, vp, i64,
                                              vp, vp, vp, vp, vp]),
        'wn_test_align_dp_host': (ctypes.c_int, [i32, vp, i32, i32, ctypes.POINTER(i32), ctypes.POINTER(i32), i32, vp, i64, vp, i64, vp, i64, vp, vp]),
        'wn_test_align_dp': (ctypes.c_int, [vp, vp, i32, i32, ctypes.POINTER(i32), ctypes.POINTER(i32), i32, vp, i64, vp, i64, vp, i64, vp, vp]),
        'wn_test_align_store_matrix': (ctypes.c_int, [vp, i32]),
        'wn_test_align_copy': (ctypes.c_int, [vp, i32, vp, i64, vp]),
    }
    for name, (res, args) in sigs.items():
        fn = getattr(lib, name)            # AttributeError here == ABI symbol missing
        fn.restype = res
        fn.argtypes = args
    lib._wn_symbols = list(sigs)
    _lib = lib
    return lib


def exported_symbols():
    return list(load_library()._wn_symbols)


def config_from_hparams(hp, max_batch, max_time, inference_only=False, grad_buckets=None):
    """hparams (reference keys, hparams.py:187-233, 309-327) -> wn_config."""
    cfg = WnConfig()
    cfg.abi_version = WN_ABI_VERSION
    for k in ('layers', 'stacks', 'residual_channels', 'gate_channels', 'skip_out_channels', 'out_channels',
              'kernel_size', 'cin_channels', 'quantize_channels', 'freq_axis_kernel_size'):
        setattr(cfg, k, int(getattr(hp, k)))
    if hp.input_type not in INPUT_TYPES:
        raise AssertionError('input_type must be one of raw / mulaw / mulaw-quantize')   # util.py:10-11
    cfg.input_type = INPUT_TYPES[hp.input_type]
    cfg.use_bias = int(bool(hp.use_bias))
    cfg.legacy = int(bool(hp.legacy))
    cfg.residual_legacy = int(bool(hp.residual_legacy))
    cfg.log_scale_min = float(hp.log_scale_min)
    cfg.log_scale_min_gauss = float(hp.log_scale_min_gauss)
    cfg.cdf_loss = int(bool(hp.cdf_loss))
    if hp.upsample_type not in UPSAMPLE_TYPES:
        raise ValueError('unknown upsample_type %r' % (hp.upsample_type,))
    cfg.upsample_type = UPSAMPLE_TYPES[hp.upsample_type]
    cfg.upsample_activation = ACTIVATIONS[hp.upsample_activation]
    scales = list(hp.upsample_scales)
    if hp.upsample_type == 'NearestNeighbor':
        from datasets.audio import get_hop_size
        scales = [get_hop_size(hp)]
    cfg.n_upsample = len(scales)
    for i, s in enumerate(scales):
        cfg.upsample_scales[i] = int(s)
    cfg.leaky_alpha = float(hp.leaky_alpha)
    cfg.dropout = float(hp.wavenet_dropout)
    cfg.clip_gradients = int(bool(hp.wavenet_clip_gradients))
    cfg.gradient_max_norm = float(hp.wavenet_gradient_max_norm)
    cfg.gradient_max_value = float(hp.wavenet_gradient_max_value)
    cfg.adam_beta1 = float(hp.wavenet_adam_beta1)
    cfg.adam_beta2 = float(hp.wavenet_adam_beta2)
    cfg.adam_epsilon = float(hp.wavenet_adam_epsilon)
    cfg.ema_decay = float(hp.wavenet_ema_decay)
    cfg.max_batch = int(max_batch)
    cfg.max_time = int(max_time)
    cfg.gin_channels = int(getattr(hp, 'gin_channels', -1))                       # hparams.py:228-230
    cfg.use_speaker_embedding = int(bool(getattr(hp, 'use_speaker_embedding', True))) if cfg.gin_channels > 0 else 0
    cfg.n_speakers = int(getattr(hp, 'n_speakers', 0) or 0)
    cfg.weight_normalization = int(bool(getattr(hp, 'wavenet_weight_normalization', False)))      # hparams.py:323
    cfg.inference_only = int(bool(inference_only))
    if grad_buckets is None:      # data parallel: 3 pieces (two early layer groups + the rest) overlap the all-reduce with the backward; single GPU: 1
        import torch
        dp = torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1
        grad_buckets = int(getattr(hp, 'mi355_grad_buckets', 3)) if dp else 1
    cfg.grad_buckets = int(grad_buckets)
    dt = str(getattr(hp, 'mi355_compute_dtype', 'bf16'))
    if dt not in COMPUTE_DTYPES:
        raise ValueError("mi355_compute_dtype must be 'bf16' or 'fp32' (got %r)" % (dt,))
    cfg.compute_dtype = COMPUTE_DTYPES[dt]
    return cfg


def _ptr(t):
    return ctypes.c_void_p(0) if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _check(t, dtype, name):
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise TypeError('%s must be a CUDA(HIP) tensor' % name)
    if t.dtype != dtype:
        raise TypeError('%s must have dtype %s (got %s)' % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise ValueError('%s must be contiguous' % name)
    return t


class Engine:
    """One wn_ctx: owns packed weights + workspace on the current device."""

    def __init__(self, hp, max_batch, max_time, inference_only=False, grad_buckets=None):
        """inference_only: synthesis-only context (no training workspace, every synthesis buffer pre-sized: wn_config.inference_only).
        grad_buckets: pieces of the flat gradient train_bwd completes early (None: 3 under torch.distributed with > 1 rank, else 1)."""
        self.lib = load_library()
        self.cfg = config_from_hparams(hp, max_batch, max_time, inference_only, grad_buckets)
        h = ctypes.c_void_p()
        rc = self.lib.wn_create(ctypes.byref(self.cfg), ctypes.byref(h))
        if rc != 0:
            raise WnError(rc, (self.lib.wn_last_error(None) or b'').decode())
        self.h = h
        self.hop = int(np.prod([self.cfg.upsample_scales[i] for i in range(self.cfg.n_upsample)]))
        self.n_params = int(self.lib.wn_param_count(self.h))
        self.layout = OrderedDict()
        name = ctypes.create_string_buffer(128)
        shape = (ctypes.c_int32 * 4)()
        ndim = ctypes.c_int32()
        off = ctypes.c_int64()
        for i in range(self.lib.wn_num_tensors(self.h)):
            self._ok(self.lib.wn_tensor_info(self.h, i, name, shape, ctypes.byref(ndim), ctypes.byref(off)))
            self.layout[name.value.decode()] = (tuple(shape[k] for k in range(ndim.value)), int(off.value))

    def set_global_condition(self, g):
        """g: int32 speaker ids [B] (use_speaker_embedding) or float32 [B, gin_channels]; applies to the next forward / synthesis
        (wavenet.py:669-678, 766-777)."""
        import torch
        g = g.contiguous()
        want = torch.int32 if self.cfg.use_speaker_embedding else torch.float32
        _check(g, want, 'g')
        self._ok(self.lib.wn_set_global_condition(self.h, _ptr(g), int(g.shape[0]), _stream()))

    def close(self):
        if getattr(self, 'h', None):
            self.lib.wn_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ok(self, rc):
        if rc != 0:
            raise WnError(rc, (self.lib.wn_last_error(self.h) or b'').decode())

    # ---- parameter helpers
    def views(self, flat):
        """name -> view into the flat fp32 buffer (TF layouts)."""
        out = OrderedDict()
        for k, (shape, off) in self.layout.items():
            out[k] = flat[off:off + int(np.prod(shape))].view(*shape)
        return out

    @property
    def receptive_field(self):
        return int(self.lib.wn_receptive_field(self.h))

    @property
    def noise_per_step(self):
        return int(self.lib.wn_noise_per_step(self.h))

    # ---- hot path
    def pack_weights(self, params):
        import torch
        _check(params, torch.float32, 'params')
        self._ok(self.lib.wn_pack_weights(self.h, _ptr(params), _stream()))

    def train_fwd(self, x, c, y, lengths, dropout_seed, loss_out, y_hat_out=None):
        import torch
        B, T = int(lengths.shape[0]), int(x.shape[-1])
        Tc = int(c.shape[-1])
        _check(c, torch.float32, 'c'); _check(lengths, torch.int32, 'lengths')
        self._ok(self.lib.wn_train_fwd(self.h, _ptr(x), _ptr(c), _ptr(y), _ptr(lengths), B, T, Tc,
                                       ctypes.c_uint64(int(dropout_seed) & (2 ** 64 - 1)), _ptr(loss_out), _ptr(y_hat_out), _stream()))

    def train_bwd(self, grads):
        import torch
        _check(grads, torch.float32, 'grads')
        self._ok(self.lib.wn_train_bwd(self.h, _ptr(grads), _stream()))

    def grad_buckets(self):
        """[(offset, count)] of the pieces in which train_bwd completes the flat gradient buffer (top layers first)."""
        out = []
        off, cnt = ctypes.c_int64(), ctypes.c_int64()
        for i in range(int(self.lib.wn_bwd_num_buckets(self.h))):
            self._ok(self.lib.wn_bwd_bucket_range(self.h, i, ctypes.byref(off), ctypes.byref(cnt)))
            out.append((int(off.value), int(cnt.value)))
        return out

    def wait_bucket(self, i, stream):
        """Order `stream` (a torch.cuda.Stream) after bucket i of the last train_bwd."""
        self._ok(self.lib.wn_bwd_wait_bucket(self.h, int(i), ctypes.c_void_p(stream.cuda_stream)))

    def optim_step(self, params, grads, m, v, ema, lr, step):
        self._ok(self.lib.wn_optim_step(self.h, _ptr(params), _ptr(grads), _ptr(m), _ptr(v), _ptr(ema),
                                        ctypes.c_float(lr), ctypes.c_int64(step), _stream()))

    def upsampled_features(self, out):
        self._ok(self.lib.wn_get_upsampled_features(self.h, _ptr(out), _stream()))

    def synthesize(self, c, noise, out_samples, out_raw=None, test_inputs=None, steps_per_graph=0, seed=0):
        """Enqueue the generation of T = Tc*hop samples for B streams (asynchronous: call synth_check() after synchronising).
        noise None: drawn on the device from `seed` (Philox4x32-10; fill_noise gives the same stream).  steps_per_graph <= 0: the
        persistent pipeline when the model fits it, else the launch-per-layer hipGraph path; > 0: that path with this many steps
        per captured graph."""
        B, Tc = int(c.shape[0]), int(c.shape[-1])
        self._ok(self.lib.wn_synthesize(self.h, _ptr(c), B, Tc, _ptr(noise), ctypes.c_uint64(int(seed) & (2 ** 64 - 1)), _ptr(test_inputs),
                                        _ptr(out_samples), _ptr(out_raw), int(steps_per_graph), _stream()))

    def synthesize_wide(self, c, noise, out_samples, out_raw=None, test_inputs=None, steps_per_graph=0, seed=0):
        """synthesize() for any B <= max_batch (wn_synthesize_wide): always the launch-per-layer path, ceil(B / 32) tiles of streams per
        launch; steps_per_graph <= 0 means 32.  A stream's samples do not depend on B: B <= 32 is synthesize(steps_per_graph > 0) bit for bit."""
        B, Tc = int(c.shape[0]), int(c.shape[-1])
        self._ok(self.lib.wn_synthesize_wide(self.h, _ptr(c), B, Tc, _ptr(noise), ctypes.c_uint64(int(seed) & (2 ** 64 - 1)), _ptr(test_inputs),
                                             _ptr(out_samples), _ptr(out_raw), int(steps_per_graph), _stream()))

    # ---- streaming synthesis (wn_synth_stream_*): the samples of one synthesize() over the concatenated frames, push by push
    def stream_lookahead(self):
        """(frames_left, frames_right) of mel context the upsample net needs around a frame: a push generates the frames
        [done, pushed - frames_right) (all of them with final=True)."""
        return stream_lookahead(self.cfg)

    def stream_begin(self, B, seed=0, steps_per_graph=0):
        """Open a stream of B utterances at t = 0 (path as synthesize(steps_per_graph) would take for B; global conditioning as set)."""
        self._stream_B = None
        self._ok(self.lib.wn_synth_stream_begin(self.h, int(B), ctypes.c_uint64(int(seed) & (2 ** 64 - 1)), int(steps_per_graph), _stream()))
        self._stream_B = int(B)

    def stream_end(self):
        """Abandon the open stream (a later stream_push raises WN_E_STATE)."""
        self._stream_B = None
        self._ok(self.lib.wn_synth_stream_end(self.h))

    def stream_push(self, c, out_samples, out_raw=None, noise=None, test_inputs=None, final=False):
        """Append c [B, cin, Tn] (None: no frames) and enqueue every sample whose conditioning is complete into out_samples [B, >= n]
        (contiguous [B, n] view expected), out_raw [B, O, n]; returns n (known without synchronising)."""
        import torch
        Tn = 0 if c is None else int(c.shape[-1])
        B = getattr(self, '_stream_B', None)
        if c is not None:
            _check(c, torch.float32, 'c')
            if B is not None and tuple(c.shape) != (B, self.cfg.cin_channels, Tn):
                raise ValueError('stream_push: c must be [B=%d, cin=%d, Tn] (got %s)' % (B, self.cfg.cin_channels, tuple(c.shape)))
        n = ctypes.c_int32(0)
        self._ok(self.lib.wn_synth_stream_push(self.h, _ptr(c), Tn, 1 if final else 0, _ptr(noise), _ptr(test_inputs), _ptr(out_samples),
                                               _ptr(out_raw), ctypes.byref(n), _stream()))
        return int(n.value)

    # ---- synthesis slots (wn_synth_slots_*): B independent utterances that join and leave one running batch
    def slots_begin(self, B, steps_per_graph=0):
        """Open a session of B idle slots (path as synthesize(steps_per_graph) would take for B, kept for the session)."""
        self._slots_B = None
        self._ok(self.lib.wn_synth_slots_begin(self.h, int(B), int(steps_per_graph), _stream()))
        self._slots_B = int(B)

    def wide_slots_begin(self, B, steps_per_graph=0):
        """Open a session of B idle slots for any B <= max_batch (wn_synth_wide_slots_begin): always the launch-per-layer path, ceil(B / 32) tiles of
        slots per launch; steps_per_graph <= 0 means 32.  Every other slot call serves it as it serves slots_begin's session."""
        self._slots_B = None
        self._ok(self.lib.wn_synth_wide_slots_begin(self.h, int(B), int(steps_per_graph), _stream()))
        self._slots_B = int(B)

    def slot_open(self, slot, seed=0, g=None):
        """The slot carries a new utterance from its own t = 0 with the next push.  g: this utterance's global condition, a CUDA tensor with one
        int32 speaker id (use_speaker_embedding) or float32 [gin_channels]; None iff the model has no global conditioning."""
        import torch
        if g is not None:
            g = g.contiguous()
            _check(g, torch.int32 if self.cfg.use_speaker_embedding else torch.float32, 'g')
            self._slot_g = getattr(self, '_slot_g', {})
            self._slot_g[int(slot)] = g          # (the library reads it in stream order)
        self._ok(self.lib.wn_synth_slot_open(self.h, int(slot), ctypes.c_uint64(int(seed) & (2 ** 64 - 1)), _ptr(g), _stream()))

    def slots_push(self, c, frames, final, out_samples, out_raw=None, noise=None, test_inputs=None):
        """c [B, cin, Tn] (None: no frames); frames[b] leading frames of row b go to slot b, final[b]: its utterance ends.  out_samples
        [B, pitch] / out_raw [B, O, pitch] / test_inputs [B, pitch] (contiguous); returns the list n_out[b] (known without synchronising)."""
        import torch
        B = self._slots_B if getattr(self, '_slots_B', None) else len(frames)
        Tn = 0 if c is None else int(c.shape[-1])
        if c is not None:
            _check(c, torch.float32, 'c')
            if tuple(c.shape) != (B, self.cfg.cin_channels, Tn):
                raise ValueError('slots_push: c must be [B=%d, cin=%d, Tn] (got %s)' % (B, self.cfg.cin_channels, tuple(c.shape)))
        if len(frames) != B or len(final) != B:
            raise ValueError('slots_push: frames / final must have one entry per slot (%d)' % B)
        pitch = 0 if out_samples is None else int(out_samples.shape[-1])
        for t, name in ((out_samples, 'out_samples'), (out_raw, 'out_raw'), (test_inputs, 'test_inputs')):
            if t is not None and (not t.is_contiguous() or int(t.shape[-1]) != pitch or int(t.shape[0]) != B):
                raise ValueError('slots_push: %s must be contiguous [B, ..., pitch=%d]' % (name, pitch))
        fr = (ctypes.c_int32 * B)(*[int(v) for v in frames])
        fi = (ctypes.c_int32 * B)(*[1 if v else 0 for v in final])
        n = (ctypes.c_int32 * B)()
        self._ok(self.lib.wn_synth_slots_push(self.h, _ptr(c), Tn, fr, fi, _ptr(noise), _ptr(test_inputs), _ptr(out_samples), _ptr(out_raw), pitch, n, _stream()))
        return [int(v) for v in n]

    def slot_abandon(self, slot):
        self._ok(self.lib.wn_synth_slot_abandon(self.h, int(slot)))

    def slot_frames_done(self, slot):
        """Frames generated so far for the slot's utterance, -1 for an idle slot."""
        rc = int(self.lib.wn_synth_slot_frames_done(self.h, int(slot)))
        if rc < -1:
            self._ok(rc)
        return rc

    def slots_end(self):
        self._slots_B = None
        self._ok(self.lib.wn_synth_slots_end(self.h))

    # ---- folded synthesis (wn_synthesize_folded): utterances cut into overlapping rows that run side by side and are cross-faded back
    def synthesize_folded(self, c, utt_frames, rows, out_wav, fade_kind='equal_power', g=None, noise=None, seed=0, test_inputs=None, out_rows=None, out_raw=None,
                          steps_per_graph=0):
        """c float32 [U, cin, F_max]; utt_frames: U ints; rows: the plan, (utt, first, frames, keep, fade) tuples (fold_plan); out_wav float32 [U, wav_pitch]
        receives the decoded, cross-faded waveforms.  Optional: g (int32 [U] speaker ids / float32 [U, gin]), noise [n_max, n_rows, nps], test_inputs
        [U, wav_pitch] (model domain), out_rows [n_rows, row_pitch] / out_raw [n_rows, O, row_pitch].  Asynchronous, as synthesize()."""
        import torch
        _check(c, torch.float32, 'c'); _check(out_wav, torch.float32, 'out_wav')
        U, n_rows = len(utt_frames), len(rows)
        if c.dim() != 3 or int(c.shape[0]) != U or int(c.shape[1]) != self.cfg.cin_channels or int(c.shape[2]) != max(int(f) for f in utt_frames):
            raise ValueError('synthesize_folded: c must be [U=%d, cin=%d, F_max=%d] (got %s)' % (U, self.cfg.cin_channels, max(int(f) for f in utt_frames), tuple(c.shape)))
        if out_wav.dim() != 2 or int(out_wav.shape[0]) != U:
            raise ValueError('synthesize_folded: out_wav must be [U=%d, wav_pitch]' % U)
        wav_pitch = int(out_wav.shape[1])
        if test_inputs is not None and (not test_inputs.is_contiguous() or tuple(test_inputs.shape) != (U, wav_pitch)):
            raise ValueError('synthesize_folded: test_inputs must be contiguous [U=%d, wav_pitch=%d]' % (U, wav_pitch))
        row_pitch = 0
        for t, name in ((out_rows, 'out_rows'), (out_raw, 'out_raw')):
            if t is None:
                continue
            if not t.is_contiguous() or int(t.shape[0]) != n_rows or (row_pitch and int(t.shape[-1]) != row_pitch):
                raise ValueError('synthesize_folded: %s must be contiguous [n_rows=%d, ..., row_pitch]' % (name, n_rows))
            row_pitch = int(t.shape[-1])
        if g is not None:
            g = g.contiguous()
            _check(g, torch.int32 if self.cfg.use_speaker_embedding else torch.float32, 'g')
        if fade_kind not in FADE_KINDS:
            raise ValueError("fade_kind must be 'equal_power' or 'linear' (got %r)" % (fade_kind,))
        uf = (ctypes.c_int32 * U)(*[int(f) for f in utt_frames])
        rw = _fold_rows(rows)
        self._ok(self.lib.wn_synthesize_folded(self.h, _ptr(c), uf, U, rw, n_rows, FADE_KINDS[fade_kind], _ptr(g), _ptr(noise), ctypes.c_uint64(int(seed) & (2 ** 64 - 1)),
                                               _ptr(test_inputs), _ptr(out_wav), wav_pitch, _ptr(out_rows), _ptr(out_raw), row_pitch, int(steps_per_graph), _stream()))

    def fill_noise(self, noise, B, T, seed):
        """The device noise stream of synthesize(noise=None, seed): float32 [T, B, noise_per_step]."""
        import torch
        _check(noise, torch.float32, 'noise')
        self._ok(self.lib.wn_fill_noise(self.h, _ptr(noise), int(B), int(T), ctypes.c_uint64(int(seed) & (2 ** 64 - 1)), _stream()))
        return noise

    # ---- sampling temperature (wn_synth_set_temperature ...): a pair (tau_scale: the logistic / normal draw, tau_select: the Gumbel choices)
    def set_temperature(self, tau_scale=1.0, tau_select=1.0):
        """Sampling temperature of the next synthesize() / stream pushes / slots opened from now on (host state; (1, 1) at creation; each in
        [0, 2]; 0: the deterministic decode).  Ends no stream or session."""
        self._ok(self.lib.wn_synth_set_temperature(self.h, float(tau_scale), float(tau_select)))

    @property
    def temperature(self):
        """(tau_scale, tau_select) of the context."""
        a, b = ctypes.c_float(), ctypes.c_float()
        self._ok(self.lib.wn_synth_get_temperature(self.h, ctypes.byref(a), ctypes.byref(b)))
        return float(a.value), float(b.value)

    def slot_temperature(self, slot, tau_scale=1.0, tau_select=1.0):
        """Override the pair of a LIVE slot (slot_open copied the context's), from the next push on."""
        self._ok(self.lib.wn_synth_set_slot_temperature(self.h, int(slot), float(tau_scale), float(tau_select)))

    def temper_noise(self, noise, tau_scale=1.0, tau_select=1.0, out=None):
        """noise float32 [T, B, noise_per_step] tempered into `out` (None: a new tensor; `noise` itself: in place).  fill_noise + temper_noise
        reproduce a device-noise run at a temperature with an explicit buffer at (1, 1), bit for bit."""
        import torch
        _check(noise, torch.float32, 'noise')
        if noise.dim() != 3 or int(noise.shape[2]) != self.noise_per_step:
            raise ValueError('temper_noise: noise must be [T, B, noise_per_step=%d] (got %s)' % (self.noise_per_step, tuple(noise.shape)))
        if out is None:
            out = torch.empty_like(noise)
        _check(out, torch.float32, 'out')
        if tuple(out.shape) != tuple(noise.shape):
            raise ValueError('temper_noise: out must have the shape of noise')
        self._ok(self.lib.wn_temper_noise(self.h, _ptr(noise), _ptr(out), int(noise.shape[1]), int(noise.shape[0]), float(tau_scale), float(tau_select), _stream()))
        return out

    def fill_noise_tempered(self, noise, B, T, seed, tau_scale, tau_select):
        """Test hook: the fill synthesize(noise=None, seed) runs at a pair, alone (== fill_noise + temper_noise, bit for bit)."""
        import torch
        _check(noise, torch.float32, 'noise')
        self._ok(self.lib.wn_test_fill_noise_tempered(self.h, _ptr(noise), int(B), int(T), ctypes.c_uint64(int(seed) & (2 ** 64 - 1)), float(tau_scale), float(tau_select), _stream()))
        return noise

    def synth_check(self):
        """Wait for the last synthesize of this engine and raise if the pipeline gave up on a hand-off."""
        self._ok(self.lib.wn_synth_check(self.h))

    def pipeline_eligible(self, B):
        """Would synthesize(steps_per_graph <= 0) run B streams on the persistent pipeline?"""
        rc = int(self.lib.wn_synth_pipe_eligible(self.h, int(B)))
        if rc < 0:
            self._ok(rc)
        return rc == 1

    def pipeline_dtype(self, half):
        """16-bit storage type of the persistent pipeline for the next runs: True = IEEE half (default), False = bf16."""
        self._ok(self.lib.wn_synth_pipe_dtype(self.h, 1 if half else 0))

    def synth_config(self):
        """How the last synthesize() ran, as the library configured it (wn_synth_last_config)."""
        v = (ctypes.c_int32 * 10)()
        n = int(self.lib.wn_synth_last_config(self.h, v, 10))
        if n < 0:
            self._ok(n)
        keys = ('path', 'instances', 'batched_premultiplication', 'kernel_spec', 'half_storage', 'head_cus', 'early_from', 'abort_every', 'workgroups', 'streams_per_instance')
        d = dict(zip(keys, (int(v[i]) for i in range(n))))
        d['path'] = {0: None, 1: 'graph', 2: 'pipeline', 3: 'graph-fp32'}.get(d.get('path'))
        return d

    @property
    def synth_path(self):
        return {0: None, 1: 'graph', 2: 'pipeline', 3: 'graph-fp32'}.get(int(self.lib.wn_synth_last_path(self.h)))

    def loss(self, y_hat, y, lengths, shift, loss_out):
        B, T = int(y_hat.shape[0]), int(y_hat.shape[-1])
        self._ok(self.lib.wn_loss(self.h, _ptr(y_hat), _ptr(y), _ptr(lengths), B, T, int(shift), _ptr(loss_out), _stream()))

    def eval_fwd(self, x, c, y, lengths, stats_out, nll_out=None, y_hat_out=None):
        """Teacher-forced forward WITHOUT dropout (whatever wavenet_dropout is) + scores: stats_out float32 [B, 3] = (sum of the negative
        log-likelihood, counted positions, counted positions with a non-zero loss) per utterance, nll_out optional [B, T] per sample,
        y_hat_out optional [B, O, T].  Saves nothing for a backward (train_bwd raises until the next train_fwd)."""
        import torch
        B, T = int(lengths.shape[0]), int(x.shape[-1])
        Tc = int(c.shape[-1])
        _check(c, torch.float32, 'c'); _check(lengths, torch.int32, 'lengths')
        self._score_outputs(B, T, stats_out, nll_out)
        if y_hat_out is not None:
            _check(y_hat_out, torch.float32, 'y_hat_out')
        self._ok(self.lib.wn_eval_fwd(self.h, _ptr(x), _ptr(c), _ptr(y), _ptr(lengths), B, T, Tc, _ptr(stats_out), _ptr(nll_out), _ptr(y_hat_out), _stream()))

    def score(self, y_hat, y, lengths, shift, stats_out, nll_out=None):
        """Scores of [B, O, T] head outputs against y (shift as loss()): stats_out / nll_out as eval_fwd.  No gradient is written: works on
        inference-only engines and leaves a pending train_bwd valid."""
        import torch
        _check(y_hat, torch.float32, 'y_hat'); _check(lengths, torch.int32, 'lengths')
        B, T = int(y_hat.shape[0]), int(y_hat.shape[-1])
        self._score_outputs(B, T, stats_out, nll_out)
        self._ok(self.lib.wn_score(self.h, _ptr(y_hat), _ptr(y), _ptr(lengths), B, T, int(shift), _ptr(stats_out), _ptr(nll_out), _stream()))

    @staticmethod
    def _score_outputs(B, T, stats_out, nll_out):
        import torch
        _check(stats_out, torch.float32, 'stats_out')
        if tuple(stats_out.shape) != (B, 3):
            raise ValueError('stats_out must be [B=%d, 3] (got %s)' % (B, tuple(stats_out.shape)))
        if nll_out is not None:
            _check(nll_out, torch.float32, 'nll_out')
            if tuple(nll_out.shape) != (B, T):
                raise ValueError('nll_out must be [B=%d, T=%d] (got %s)' % (B, T, tuple(nll_out.shape)))

    def profile(self, enable):
        self._ok(self.lib.wn_profile(self.h, int(bool(enable))))

    def profile_result(self):
        ms, n = ctypes.c_double(), ctypes.c_int64()
        self._ok(self.lib.wn_profile_result(self.h, ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value

    def profile_kernel_result(self):
        """(total ms, launches) of the timed gate launches by their in-kernel start / end stamps (pure kernel time)."""
        ms, n = ctypes.c_double(), ctypes.c_int64()
        self._ok(self.lib.wn_profile_kernel_result(self.h, ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value

    def profile_kernel_clock(self):
        """(MHz, launches): mean shader clock inside the timed gate launches (workgroup 0's cycle counter over the 100 MHz wall clock)."""
        mhz, n = ctypes.c_double(), ctypes.c_int64()
        self._ok(self.lib.wn_profile_kernel_clock(self.h, ctypes.byref(mhz), ctypes.byref(n)))
        return mhz.value, n.value

    def set_batch_parts(self, parts):
        self._ok(self.lib.wn_set_batch_parts(self.h, int(parts)))

    def profile_rows_per_launch(self):
        return int(self.lib.wn_profile_rows_per_launch(self.h))

    def trace_arm(self, steps_from_now=1):
        """Stamp every tile-engine / grouped weight-gradient launch of the `steps_from_now`-th next training step (wn_trace_arm)."""
        self._ok(self.lib.wn_trace_arm(self.h, int(steps_from_now)))

    def trace_read(self, cap=1024):
        """[(kind, stream, start_tick, end_tick)] of the armed step in enqueue order, 100 MHz ticks; [] if it has not completed.  Synchronises."""
        k = (ctypes.c_int32 * cap)(); st = (ctypes.c_uint64 * cap)(); t0 = (ctypes.c_uint64 * cap)(); t1 = (ctypes.c_uint64 * cap)()
        n = self.lib.wn_trace_read(self.h, cap, k, st, t0, t1)
        if n < 0:
            self._ok(n)
        return [(int(k[i]), int(st[i]), int(t0[i]), int(t1[i])) for i in range(n)]

    def poison_workspace(self):
        """Test hook: 0xFF bytes (NaN in bf16 and fp32) over every buffer that only training steps write, whole allocations; the last forward is forgotten
        (wn_test_poison_workspace)."""
        self._ok(self.lib.wn_test_poison_workspace(self.h, _stream()))

    def debug_copy(self, name, layer, rows, cols):
        import torch
        out = torch.empty(rows, cols, dtype=torch.float32, device='cuda')
        self._ok(self.lib.wn_debug_copy(self.h, name.encode(), int(layer), _ptr(out), ctypes.c_int64(rows * cols), _stream()))
        return out

    def f32_sgemm(self, B, T, In, ld_in, W, wk, wm, K, M, Out, ld_out, shift=0, col0=0, accumulate=0, mask=None, ld_mask=0, drop_on_out=0, alpha=1.0, scale=1.0,
                  bias=None, bias_bstride=0, add=None, ld_add=0, relu=0, out_bot=0, key=(0, 0), thresh16=0, keep_scale=1.0, drop_ld=0):
        """Test hook: ONE launch of the fp32 mode's SGEMM on float32 device tensors of the caller's (wn_test_f32_sgemm; tensors may be views that
        start at any float of a buffer, the pitches are the caller's to state)."""
        import torch
        for name, t in (('In', In), ('W', W), ('Out', Out), ('mask', mask), ('bias', bias), ('add', add)):
            if t is not None:
                _check(t, torch.float32, name)
        self._ok(self.lib.wn_test_f32_sgemm(self.h, int(B), int(T), _ptr(In), int(ld_in), int(col0), int(shift), _ptr(W), int(wk), int(wm), int(K), int(M), _ptr(Out),
                                            int(ld_out), int(accumulate), _ptr(mask), int(ld_mask), int(drop_on_out), float(alpha), float(scale), _ptr(bias),
                                            int(bias_bstride), _ptr(add), int(ld_add), int(relu), int(out_bot), int(key[0]), int(key[1]), int(thresh16),
                                            float(keep_scale), int(drop_ld), _stream()))

    def f32_wgrad(self, B, T, A, lda, K, Bm, ldb, M, out, ldo, shift=0, alpha=1.0, drop_layer=-1, seed=0, bias_out=None, bias_out2=None):
        """Test hook: ONE weight gradient of the fp32 mode (launch + slab reduction) on float32 device tensors of the caller's (wn_test_f32_wgrad).
        A None: only the column sums of Bm into bias_out / bias_out2.  drop_layer >= 0: the engine's wavenet_dropout keyed by (seed, drop_layer) on A."""
        import torch
        for name, t in (('A', A), ('Bm', Bm), ('out', out), ('bias_out', bias_out), ('bias_out2', bias_out2)):
            if t is not None:
                _check(t, torch.float32, name)
        self._ok(self.lib.wn_test_f32_wgrad(self.h, int(B), int(T), _ptr(A), int(lda), int(shift), int(K), _ptr(Bm), int(ldb), int(M), _ptr(out), int(ldo), float(alpha),
                                            int(drop_layer), ctypes.c_uint64(int(seed) & (2 ** 64 - 1)), _ptr(bias_out), _ptr(bias_out2), _stream()))

    def f32_gate(self, Z, GU):
        """Test hook: the fp32 mode's gate and its derivative on Z [rows, 2 GH] and GU [rows, GH] -> (U [rows, GH], DZ [rows, 2 GH])  (wn_test_f32_gate)."""
        import torch
        _check(Z, torch.float32, 'Z'); _check(GU, torch.float32, 'GU')
        rows, GH = int(GU.shape[0]), int(GU.shape[1])
        if tuple(Z.shape) != (rows, 2 * GH):
            raise ValueError('f32_gate: Z must be [rows=%d, 2 * GH=%d] (got %s)' % (rows, 2 * GH, tuple(Z.shape)))
        U = torch.empty_like(GU); DZ = torch.empty_like(Z)
        self._ok(self.lib.wn_test_f32_gate(self.h, _ptr(Z), _ptr(GU), _ptr(U), _ptr(DZ), ctypes.c_int64(rows), GH, _stream()))
        return U, DZ

    def pack_info(self, kind, layer=0):
        """(M, K, kil, gate_interleave) of one fragment-ordered operand pack (wn_test_pack_info; tests only)."""
        out = (ctypes.c_int32 * 4)()
        self._ok(self.lib.wn_test_pack_info(self.h, kind.encode(), int(layer), out))
        return tuple(int(v) for v in out)

    def pack_copy(self, kind, layer=0):
        """One operand pack in storage order, bf16 -> fp32, flat [M * K] (wn_test_pack_copy; tests only, synchronises)."""
        import torch
        M, K, _, _ = self.pack_info(kind, layer)
        out = torch.empty(M * K, dtype=torch.float32, device='cuda')
        self._ok(self.lib.wn_test_pack_copy(self.h, kind.encode(), int(layer), _ptr(out), ctypes.c_int64(M * K)))
        return out

    def sample(self, y_hat, noise, out):
        B, T = int(y_hat.shape[0]), int(y_hat.shape[-1])
        self._ok(self.lib.wn_sample(self.h, _ptr(y_hat), B, T, _ptr(noise), _ptr(out), _stream()))


def stream_lookahead(cfg):
    """wn_synth_stream_lookahead on a WnConfig (host only: no context, no GPU)."""
    lib = load_library()
    left, right = ctypes.c_int32(), ctypes.c_int32()
    rc = lib.wn_synth_stream_lookahead(ctypes.byref(cfg), ctypes.byref(left), ctypes.byref(right))
    if rc != 0:
        raise WnError(rc, 'wn_synth_stream_lookahead: bad configuration')
    return int(left.value), int(right.value)


def _fold_rows(rows):
    arr = (WnFoldRow * max(len(rows), 1))()
    for i, r in enumerate(rows):
        arr[i].utt, arr[i].first, arr[i].frames, arr[i].keep, arr[i].fade = (int(v) for v in r)
    return arr


def fold_plan(utt_frames, rows_max, warm=4, fade=2, min_keep=40):
    """wn_fold_plan (host only: no context, no GPU): the rows of a folded run of utterances of utt_frames[u] mel frames, as (utt, first, frames, keep, fade) tuples."""
    U = len(utt_frames)
    uf = (ctypes.c_int32 * max(U, 1))(*[int(f) for f in utt_frames])
    rows = (WnFoldRow * 32)()
    n = load_library().wn_fold_plan(uf, U, int(rows_max), int(warm), int(fade), int(min_keep), rows, 32)
    if n < 0:
        raise WnError(n, 'wn_fold_plan(frames=%r, rows_max=%r, warm=%r, fade=%r, min_keep=%r)' % (list(utt_frames), rows_max, warm, fade, min_keep))
    return [(int(r.utt), int(r.first), int(r.frames), int(r.keep), int(r.fade)) for r in rows[:n]]


def fold_check(utt_frames, rows):
    """wn_fold_check (host only): raises WnError(WN_E_ARG) naming the row that breaks a rule of a folded plan."""
    U = len(utt_frames)
    uf = (ctypes.c_int32 * max(U, 1))(*[int(f) for f in utt_frames])
    msg = ctypes.create_string_buffer(400)
    rc = load_library().wn_fold_check(uf, U, _fold_rows(rows), len(rows), msg, 400)
    if rc != 0:
        raise WnError(rc, msg.value.decode())


def fold_weights(fade_kind, n):
    """(w_in, w_out) float32 [n]: the cross-fade tables wn_synthesize_folded uploads for a fade of n samples (host only)."""
    w_in, w_out = np.empty(int(n), np.float32), np.empty(int(n), np.float32)
    rc = load_library().wn_fold_weights(FADE_KINDS[fade_kind], int(n), w_in.ctypes.data_as(ctypes.c_void_p), w_out.ctypes.data_as(ctypes.c_void_p))
    if rc != 0:
        raise WnError(rc, 'wn_fold_weights(%r, %r)' % (fade_kind, n))
    return w_in, w_out


def temper_noise_host(mode, noise, tau_scale=1.0, tau_select=1.0):
    """wn_test_temper_noise: the device's tempering function evaluated on the host (no context, no GPU).  noise: float32 numpy [rows, nps];
    mode 0 MoL (nps - 1 select entries + the logistic draw), 1 Gaussian, 2 softmax.  Returns a new array."""
    a = np.ascontiguousarray(noise, dtype=np.float32)
    if a.ndim != 2:
        raise ValueError('temper_noise_host: noise must be [rows, nps]')
    out = np.empty_like(a)
    rc = load_library().wn_test_temper_noise(int(mode), int(a.shape[1]), a.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p),
                                             ctypes.c_int64(a.shape[0]), float(tau_scale), float(tau_select))
    if rc != 0:
        raise WnError(rc, 'wn_test_temper_noise(mode=%r, nps=%d, tau=(%r, %r))' % (mode, a.shape[1] if a.ndim == 2 else -1, tau_scale, tau_select))
    return out


def learning_rate(schedule, init_lr, step, decay_rate=0.5, decay_steps=200000, warmup=4000.0):
    return float(load_library().wn_learning_rate(LR_SCHEDULES[schedule], init_lr, int(step), decay_rate, int(decay_steps), warmup))


# ---- mu-law codec on device tensors (wavenet_vocoder/util.py semantics, mu = 255)
def _ew(fn_name, src, dst):
    lib = load_library()
    rc = getattr(lib, fn_name)(_ptr(src), _ptr(dst), ctypes.c_int64(src.numel()), _stream())
    if rc != 0:
        raise WnError(rc, (lib.wn_last_error(None) or b'').decode())
    return dst


def mulaw(x):
    import torch
    return _ew('wn_mulaw', _check(x, torch.float32, 'x'), torch.empty_like(x))


def inv_mulaw(y):
    import torch
    return _ew('wn_inv_mulaw', _check(y, torch.float32, 'y'), torch.empty_like(y))


def mulaw_quantize(x):
    import torch
    return _ew('wn_mulaw_quantize', _check(x, torch.float32, 'x'), torch.empty(x.shape, dtype=torch.int32, device=x.device))


def inv_mulaw_quantize(q):
    import torch
    return _ew('wn_inv_mulaw_quantize', _check(q, torch.int32, 'q'), torch.empty(q.shape, dtype=torch.float32, device=q.device))


def argmax_channels(logits):
    import torch
    _check(logits, torch.float32, 'logits')
    B, Q, T = logits.shape
    out = torch.empty(B, T, dtype=torch.int32, device=logits.device)
    lib = load_library()
    rc = lib.wn_argmax_channels(_ptr(logits), _ptr(out), B, Q, T, _stream())
    if rc != 0:
        raise WnError(rc, (lib.wn_last_error(None) or b'').decode())
    return out


def mel_config_from_hparams(hp, max_batch, max_samples, preemphasis=0.0):
    """hparams (reference keys, hparams.py:102-133) -> wn_mel_config.  preemphasis: the k fused into the read of the signal (0: the
    analysed signal is the input itself, the contract of datasets.audio.melspectrogram)."""
    from datasets.audio import get_hop_size
    cfg = WnMelConfig()
    cfg.abi_version = WN_ABI_VERSION
    cfg.sample_rate = int(hp.sample_rate)
    cfg.n_fft = int(hp.n_fft)
    cfg.hop_size = int(get_hop_size(hp))
    cfg.win_size = int(hp.n_fft if hp.win_size is None else hp.win_size)
    cfg.num_mels = int(hp.num_mels)
    cfg.magnitude_power = float(hp.magnitude_power)
    cfg.min_level_db = float(hp.min_level_db)
    cfg.ref_level_db = float(hp.ref_level_db)
    cfg.max_abs_value = float(hp.max_abs_value)
    cfg.preemphasis = float(preemphasis)
    cfg.signal_normalization = int(bool(hp.signal_normalization))
    cfg.allow_clipping = int(bool(hp.allow_clipping_in_normalization))
    cfg.symmetric_mels = int(bool(hp.symmetric_mels))
    cfg.max_batch = int(max_batch)
    cfg.max_samples = int(max_samples)
    return cfg


class MelAnalyzer:
    """One wn_mel: wav -> mel-spectrogram on the current device (csrc/wn_mel.hip; replaces datasets.audio.melspectrogram's numpy / the
    reference's librosa on the preprocessing path).  max_batch = 0 gives a geometry-only analyzer (num_frames; no device)."""

    def __init__(self, hparams, max_batch, max_samples, preemphasis=0.0, mel_basis=None):
        """preemphasis: k of y[s] = x[s] - k x[s - 1] fused into run() and peak() (0: off).  mel_basis: [num_mels, 1 + n_fft // 2]
        (default datasets.audio._build_mel_basis(hparams) == librosa.filters.mel)."""
        if getattr(hparams, 'use_lws', False):
            raise NotImplementedError('use_lws: the lws package is not available')
        self.lib = load_library()
        self.cfg = mel_config_from_hparams(hparams, max_batch, max_samples, preemphasis)
        if mel_basis is None:
            from datasets.audio import _build_mel_basis
            mel_basis = _build_mel_basis(hparams)
        mb = np.ascontiguousarray(mel_basis, dtype=np.float32)
        if mb.shape != (self.cfg.num_mels, 1 + self.cfg.n_fft // 2):
            raise ValueError('mel_basis must be [num_mels, 1 + n_fft // 2] = %r (got %r)' % ((self.cfg.num_mels, 1 + self.cfg.n_fft // 2), mb.shape))
        h = ctypes.c_void_p()
        rc = self.lib.wn_mel_create(ctypes.byref(self.cfg), mb.ctypes.data_as(ctypes.c_void_p), ctypes.byref(h))
        if rc != 0:
            raise WnError(rc, (self.lib.wn_mel_last_error(None) or b'').decode())
        self.h = h
        self.num_mels, self.hop = int(self.cfg.num_mels), int(self.cfg.hop_size)
        self.max_batch, self.max_samples = int(max_batch), int(max_samples)

    def _ok(self, rc):
        if rc != 0:
            raise WnError(rc, (self.lib.wn_mel_last_error(self.h) or b'').decode())

    def num_frames(self, n):
        r = int(self.lib.wn_mel_num_frames(self.h, int(n)))
        if r < 0:
            raise WnError(r, 'wn_mel_num_frames(%d)' % n)
        return r

    @property
    def frame_tile(self):
        return int(self.lib.wn_mel_frame_tile(self.h))

    def _batch(self, wav, lengths):
        import torch
        _check(wav, torch.float32, 'wav')
        if wav.dim() != 2:
            raise ValueError('wav must be [B, ld]')
        if len(lengths) != int(wav.shape[0]):
            raise ValueError('one length per row of wav (%d lengths for %d rows)' % (len(lengths), int(wav.shape[0])))
        return (ctypes.c_int32 * len(lengths))(*[int(n) for n in lengths])

    def peak(self, wav, lengths, out=None):
        """max |x[s] - k x[s - 1]| per utterance -> float32 [B] on the device."""
        import torch
        lens = self._batch(wav, lengths)
        if out is None:
            out = torch.empty(wav.shape[0], dtype=torch.float32, device=wav.device)
        _check(out, torch.float32, 'out')
        self._ok(self.lib.wn_mel_peak(self.h, _ptr(wav), int(wav.shape[1]), lens, len(lens), _ptr(out), _stream()))
        return out

    def run(self, wav, lengths, gain=None, channels_first=False, frames=None, out=None):
        """wav float32 [B, ld] on the device, lengths: B ints (host) -> [B, F_max, num_mels] (channels_first: [B, num_mels, F_max]) on the
        device; F_max = frames or the frames of the longest utterance; rows past an utterance's frames hold the zero-signal value."""
        import torch
        lens = self._batch(wav, lengths)
        B = len(lens)
        if gain is not None:
            _check(gain, torch.float32, 'gain')
            if gain.numel() != B:
                raise ValueError('gain must be [B]')
        F = int(frames) if frames is not None else max(1 + int(n) // self.hop for n in lens)
        shape = (B, self.num_mels, F) if channels_first else (B, F, self.num_mels)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=wav.device)
        _check(out, torch.float32, 'out')
        if tuple(out.shape) != shape:
            raise ValueError('out must be %r' % (shape,))
        self._ok(self.lib.wn_mel_run(self.h, _ptr(wav), int(wav.shape[1]), lens, _ptr(gain), _ptr(out), B, F, int(bool(channels_first)), _stream()))
        return out

    def close(self):
        if getattr(self, 'h', None):
            self.lib.wn_mel_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- streaming mel analysis (csrc/wn_mel_stream.hip)
def mel_stream_geometry(n_fft, win_size, hop):
    """(Hl, Hr) of the frames: frame f reads the samples [f hop - Hl, f hop + Hr)."""
    off = (int(n_fft) - int(win_size)) // 2
    Hl = int(n_fft) // 2 - off
    return Hl, int(win_size) - Hl


def mel_stream_ready(n_fft, win_size, hop, S, final=False):
    """The rule of readiness in Python (what wn_mel_stream_ready computes): frames analysed of a row that was given S samples since its restart."""
    S, hop = int(S), int(hop)
    Hr = mel_stream_geometry(n_fft, win_size, hop)[1]
    if final:
        return 1 + S // hop
    return (S - Hr) // hop + 1 if S >= Hr else 0


def mel_stream_plan(stream, pushes, in_pitch=None, out_pitch=None, have_in=True):
    """wn_test_mel_stream_plan on a geometry-only MelStream: pushes is a list of (n [B], restart [B] or None, final [B] or None).  Returns a dict of numpy arrays:
    status [P], and [P, B] n_out, first_frame, tail_len, S, F (the counters after each push; a refused push changes none)."""
    vp = ctypes.c_void_p
    P, B = len(pushes), len(pushes[0][0])
    n = np.zeros((P, B), np.int32); rs = np.zeros((P, B), np.int32); fin = np.zeros((P, B), np.int32)
    for p, (nn, r, f) in enumerate(pushes):
        n[p] = nn
        if r is not None:
            rs[p] = np.asarray(r, np.int32)
        if f is not None:
            fin[p] = np.asarray(f, np.int32)
    ipitch = int(max(1, n.max())) if in_pitch is None else int(in_pitch)
    opitch = int(n.max()) // stream.hop + 3 if out_pitch is None else int(out_pitch)
    res = {'status': np.full(P, -99, np.int32), 'n_out': np.full((P, B), -1, np.int32), 'first_frame': np.full((P, B), -1, np.int64),
           'tail_len': np.full((P, B), -1, np.int32), 'S': np.full((P, B), -1, np.int64), 'F': np.full((P, B), -1, np.int64)}
    dummy = np.zeros(1, np.float32)
    lib = load_library()
    rc = lib.wn_test_mel_stream_plan(stream.h, dummy.ctypes.data_as(vp) if have_in else None, ipitch, n.ctypes.data_as(vp), rs.ctypes.data_as(vp), fin.ctypes.data_as(vp), P, B, opitch,
                                     *[res[k].ctypes.data_as(vp) for k in ('status', 'n_out', 'first_frame', 'tail_len', 'S', 'F')])
    if rc != 0:
        raise WnError(rc, (lib.wn_mel_stream_last_error(None) or b'').decode())
    return res


class MelStream:
    """One wn_mel_stream: MelAnalyzer.run on rows that arrive push by push on the current device (csrc/wn_mel_stream.hip), asynchronously.  A row's frames,
    concatenated, are bit-identical to MelAnalyzer.run on the whole row with the same gain and pre-emphasis; they lag the samples given by lag_samples = Hr
    (ready()).  rows = 0: a geometry-only handle that needs no GPU.  Use one handle from one stream at a time."""

    def __init__(self, hparams, rows, max_push, preemphasis=0.0, mel_basis=None):
        if getattr(hparams, 'use_lws', False):
            raise NotImplementedError('use_lws: the lws package is not available')
        self.lib = load_library()
        self.cfg = mel_config_from_hparams(hparams, 0, 0, preemphasis)
        if mel_basis is None:
            from datasets.audio import _build_mel_basis
            mel_basis = _build_mel_basis(hparams)
        mb = np.ascontiguousarray(mel_basis, dtype=np.float32)
        if mb.shape != (self.cfg.num_mels, 1 + self.cfg.n_fft // 2):
            raise ValueError('mel_basis must be [num_mels, 1 + n_fft // 2] = %r (got %r)' % ((self.cfg.num_mels, 1 + self.cfg.n_fft // 2), mb.shape))
        h = ctypes.c_void_p()
        rc = self.lib.wn_mel_stream_create(ctypes.byref(self.cfg), mb.ctypes.data_as(ctypes.c_void_p), int(rows), int(max_push), ctypes.byref(h))
        if rc != 0:
            raise WnError(rc, (self.lib.wn_mel_stream_last_error(None) or b'').decode())
        self.h = h
        self.num_mels, self.hop = int(self.cfg.num_mels), int(self.cfg.hop_size)
        self.rows, self.max_push = int(rows), int(max_push)
        self.lead_samples, self.lag_samples = mel_stream_geometry(self.cfg.n_fft, self.cfg.win_size, self.hop)

    def _ok(self, rc):
        if rc != 0:
            raise WnError(rc, (self.lib.wn_mel_stream_last_error(self.h) or b'').decode())

    def ready(self, S, final=False):
        r = int(self.lib.wn_mel_stream_ready(self.h, int(S), int(bool(final))))
        if r < 0:
            raise WnError(r, 'wn_mel_stream_ready(%d)' % S)
        return r

    def push(self, samples, n=None, restart=None, final=None, gain=None, channels_first=True, out=None):
        """samples [B, pitch] float32 on the device, n: B ints (None: the whole pitch), restart / final: B flags (None: none; True: all), gain: B host floats read
        where restart is set (None: 1).  Returns (mel float32 [B, num_mels, pitch'] -- channels_first False: [B, pitch', num_mels] -- on the device, n_out: B
        ints): row b's next n_out[b] frames, zeros beyond (with out given: its bytes kept)."""
        import torch
        _check(samples, torch.float32, 'samples')
        if samples.dim() == 1:
            samples = samples.reshape(1, -1)
        if samples.dim() != 2:
            raise ValueError('samples must be [B, pitch]')
        B, pitch = int(samples.shape[0]), int(samples.shape[1])
        n = [pitch] * B if n is None else [int(v) for v in n]
        if len(n) != B:
            raise ValueError('one count per row of samples (%d for %d rows)' % (len(n), B))

        def flags(v, name):
            if v is None:
                return None
            f = [1] * B if v is True else [int(bool(x)) for x in v]
            if len(f) != B:
                raise ValueError('one %s flag per row' % name)
            return (ctypes.c_int32 * B)(*f)
        rs, fin = flags(restart, 'restart'), flags(final, 'final')
        if gain is not None:
            if len(gain) != B:
                raise ValueError('one gain per row')
            gain = (ctypes.c_float * B)(*[float(np.float32(g)) for g in gain])
        if out is None:
            frames = (max(max(n), 0) + self.lead_samples + self.lag_samples) // self.hop + 2      # a push adds at most the frames of n + win_size samples
            out = torch.zeros((B, self.num_mels, frames) if channels_first else (B, frames, self.num_mels), dtype=torch.float32, device=samples.device)
        _check(out, torch.float32, 'out')
        if out.dim() != 3 or int(out.shape[0]) != B or int(out.shape[1 if channels_first else 2]) != self.num_mels:
            raise ValueError('out must be [B, num_mels, pitch] (channels_first) or [B, pitch, num_mels]')
        opitch = int(out.shape[2 if channels_first else 1])
        n_out = (ctypes.c_int32 * B)()
        self._ok(self.lib.wn_mel_stream_push(self.h, _ptr(samples), pitch, (ctypes.c_int32 * B)(*n), rs, fin, gain, B, _ptr(out), opitch, int(bool(channels_first)), n_out, _stream()))
        return out, [int(v) for v in n_out]

    def close(self):
        if getattr(self, 'h', None):
            self.lib.wn_mel_stream_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def post_config(max_rows, in_type, deemphasis=0.0, gain=1.0):
    """wn_post_config.  in_type: 0 / 'raw' (a float waveform), 1 / 'mulaw', 2 / 'mulaw-quantize'."""
    cfg = WnPostConfig()
    cfg.abi_version = WN_ABI_VERSION
    cfg.max_rows = int(max_rows)
    cfg.in_type = INPUT_TYPES[in_type] if in_type in INPUT_TYPES else int(in_type)
    cfg.deemphasis = float(deemphasis)
    cfg.gain = float(gain)
    return cfg


def post_host(samples, in_type, deemphasis=0.0, carry_in=0.0, pcm_scale=32767.0):
    """wn_test_post_host: the output stage's arithmetic on the host (no handle, no GPU) over one row.  samples: numpy float32 (in_type 0 / 1) or int32 (2)
    [n].  Returns (y float32 [n], pcm int16 [n], carry_out)."""
    cfg = post_config(1, in_type, deemphasis)
    a = np.ascontiguousarray(samples, dtype=np.int32 if cfg.in_type == 2 else np.float32).reshape(-1)
    y, q, carry = np.empty(a.size, np.float32), np.empty(a.size, np.int16), ctypes.c_float(0.0)
    rc = load_library().wn_test_post_host(ctypes.byref(cfg), a.ctypes.data_as(ctypes.c_void_p), ctypes.c_int64(a.size), float(carry_in), float(pcm_scale),
                                          y.ctypes.data_as(ctypes.c_void_p), q.ctypes.data_as(ctypes.c_void_p), ctypes.byref(carry))
    if rc != 0:
        raise WnError(rc, (load_library().wn_post_last_error(None) or b'').decode())
    return y, q, np.float32(carry.value)


class OutputStage:
    """One wn_post: model-domain samples -> de-emphasised float32 and / or int16 PCM on the current device (csrc/wn_post.hip), asynchronously, with the
    filter state carried per row across push() calls: a row is bit-identical however it is cut into pushes.  Use one stage from one stream at a time."""

    def __init__(self, hparams, rows, deemphasis=None, gain=1.0, in_type=None):
        """in_type None: hparams.input_type ('raw' / 0 also takes WaveNet.folded's decoded waveforms).  deemphasis None: hparams.preemphasis if
        hparams.preemphasize else 0 (off).  gain: push() only, PCM = y * gain * 32767."""
        self.lib = load_library()
        if in_type is None:
            in_type = hparams.input_type
        if in_type not in INPUT_TYPES and in_type not in (0, 1, 2):
            raise ValueError('in_type must be one of raw / mulaw / mulaw-quantize or 0 ... 2 (got %r)' % (in_type,))
        if deemphasis is None:
            deemphasis = float(hparams.preemphasis) if hparams.preemphasize else 0.0
        self.cfg = post_config(rows, in_type, deemphasis, gain)
        h = ctypes.c_void_p()
        rc = self.lib.wn_post_create(ctypes.byref(self.cfg), ctypes.byref(h))
        if rc != 0:
            raise WnError(rc, (self.lib.wn_post_last_error(None) or b'').decode())
        self.h = h
        self.rows, self.in_type, self.deemphasis, self.gain = int(rows), int(self.cfg.in_type), float(self.cfg.deemphasis), float(self.cfg.gain)

    def _ok(self, rc):
        if rc != 0:
            raise WnError(rc, (self.lib.wn_post_last_error(self.h) or b'').decode())

    def _rows(self, samples, n):
        import torch
        _check(samples, torch.int32 if self.in_type == 2 else torch.float32, 'samples')
        if samples.dim() == 1:
            samples = samples.reshape(1, -1)
        if samples.dim() != 2:
            raise ValueError('samples must be [B, pitch]')
        B, pitch = int(samples.shape[0]), int(samples.shape[1])
        n = [pitch] * B if n is None else [int(v) for v in n]
        if len(n) != B:
            raise ValueError('one length per row of samples (%d lengths for %d rows)' % (len(n), B))
        return samples, B, pitch, n, (ctypes.c_int32 * B)(*n)

    def push(self, samples, n=None, restart=None, pcm=True, float_out=False, clipped=False):
        """samples [B, pitch] on the device (float32, or int32 class ids), n: B ints (None: the whole pitch), restart: B flags (None: none; True: all).
        Continues every row's filter where its last push left it.  Returns the int16 chunk [B, pitch] (pcm), the float32 one (float_out) and the clipped
        counts int32 [B] (clipped) -- one tensor, or a tuple in that order, on the device; elements beyond n[b] are zero."""
        import torch
        samples, B, pitch, n, nc = self._rows(samples, n)
        if not (pcm or float_out):
            raise ValueError('OutputStage.push: nothing to return (pcm and float_out are both off)')
        rs = None
        if restart is not None:
            flags = [1] * B if restart is True else [int(bool(v)) for v in restart]
            if len(flags) != B:
                raise ValueError('one restart flag per row')
            rs = (ctypes.c_int32 * B)(*flags)
        q = torch.zeros(B, pitch, dtype=torch.int16, device=samples.device) if pcm else None
        y = torch.zeros(B, pitch, dtype=torch.float32, device=samples.device) if float_out else None
        cl = torch.zeros(B, dtype=torch.int32, device=samples.device) if clipped else None
        self._ok(self.lib.wn_post_push(self.h, _ptr(samples), pitch, nc, rs, B, _ptr(y), _ptr(q), pitch, _ptr(cl), _stream()))
        res = tuple(t for t in (q, y, cl) if t is not None)
        return res[0] if len(res) == 1 else res

    def finish(self, samples, lengths, pcm=True, peak=False):
        """Whole utterances: every row from y[-1] = 0, peak-normalised as save_wavenet_wav does.  Returns (y float32 [B, pitch], int16 [B, pitch]) with pcm,
        else y; peak: also the peaks float32 [B].  The carried state of push() is neither read nor written."""
        import torch
        samples, B, pitch, n, nc = self._rows(samples, lengths)
        y = torch.zeros(B, pitch, dtype=torch.float32, device=samples.device)
        q = torch.zeros(B, pitch, dtype=torch.int16, device=samples.device) if pcm else None
        pk = torch.zeros(B, dtype=torch.float32, device=samples.device) if peak else None
        self._ok(self.lib.wn_post_finish(self.h, _ptr(samples), pitch, nc, B, _ptr(y), _ptr(q), pitch, _ptr(pk), _stream()))
        res = tuple(t for t in (y, q, pk) if t is not None)
        return res[0] if len(res) == 1 else res

    def close(self):
        if getattr(self, 'h', None):
            self.lib.wn_post_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


MELCMP_KINDS = ('bias', 'l1', 'lsd', 'mcd', 'l1c', 'lsdc')      # per_frame[b][j], and summary[b][j]; summary[b][6] is worst


def melcmp_unit_db(hp):
    """level units (dB) per unit of a mel as hparams normalise it (datasets.audio._normalize): the symmetric range spans -min_level_db over
    2 max_abs_value, the asymmetric one over max_abs_value; an unnormalised mel is in dB already."""
    if not hp.signal_normalization:
        return 1.0
    return -float(hp.min_level_db) / ((2.0 if hp.symmetric_mels else 1.0) * float(hp.max_abs_value))


def melcmp_config(num_mels, n_cep=13, unit_db=1.0, alarm_db=0.0, max_batch=0, max_frames=0):
    cfg = WnMelcmpConfig()
    cfg.abi_version = WN_ABI_VERSION
    cfg.num_mels, cfg.n_cep, cfg.unit_db, cfg.alarm_db = int(num_mels), int(n_cep), float(unit_db), float(alarm_db)
    cfg.max_batch, cfg.max_frames = int(max_batch), int(max_frames)
    return cfg


def _melcmp_geometry(t, channels_first, num_mels, name):
    if t.ndim != 3 or int(t.shape[1 if channels_first else 2]) != num_mels:
        raise ValueError('%s must be %s (got %r)' % (name, '[B, num_mels, pitch]' if channels_first else '[B, pitch, num_mels]', tuple(t.shape)))
    return int(t.shape[0]), int(t.shape[2 if channels_first else 1])


def melcmp_host(a, b, frames, num_mels=None, n_cep=13, unit_db=1.0, alarm_db=0.0, a_channels_first=True, b_channels_first=True, per_frame=True, out_pitch=None):
    """wn_test_melcmp_host: the reconstruction check on the host (no handle, no GPU), in the device's order.  a, b: numpy float32, each
    [B, num_mels, pitch] (channels_first) or [B, pitch, num_mels].  Returns a dict: summary float32 [B, 7], marks int32 [B, 2] and, with per_frame,
    per_frame float32 [B, 6, out_pitch] (elements beyond a row's frames keep the NaN they are created with)."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    M = int(a.shape[1 if a_channels_first else 2]) if num_mels is None else int(num_mels)
    B, ap = _melcmp_geometry(a, a_channels_first, M, 'a')
    B2, bp = _melcmp_geometry(b, b_channels_first, M, 'b')
    fr = [int(f) for f in frames]
    if B2 != B or len(fr) != B:
        raise ValueError('a, b and frames must have one entry per row')
    cfg = melcmp_config(M, n_cep, unit_db, alarm_db)
    op = max(fr + [0]) if out_pitch is None else int(out_pitch)
    pf = np.full((B, 6, op), np.nan, np.float32) if per_frame else None
    sm, mk = np.full((B, 7), np.nan, np.float32), np.full((B, 2), -7, np.int32)
    vp = ctypes.c_void_p
    rc = load_library().wn_test_melcmp_host(ctypes.byref(cfg), a.ctypes.data_as(vp), int(bool(a_channels_first)), ap, b.ctypes.data_as(vp), int(bool(b_channels_first)), bp,
                                            (ctypes.c_int32 * B)(*fr), B, pf.ctypes.data_as(vp) if per_frame else None, op, sm.ctypes.data_as(vp), mk.ctypes.data_as(vp))
    if rc != 0:
        raise WnError(rc, (load_library().wn_melcmp_last_error(None) or b'').decode())
    res = {'summary': sm, 'marks': mk}
    if per_frame:
        res['per_frame'] = pf
    return res


class MelCompare:
    """One wn_melcmp: distances between two mel-spectrograms per frame and per row on the current device (csrc/wn_melcmp.hip), asynchronously.
    max_batch = 0 gives a validation-only handle (no device; every run is refused)."""

    def __init__(self, num_mels, max_batch, max_frames, n_cep=13, unit_db=1.0, alarm_db=0.0):
        self.lib = load_library()
        self.cfg = melcmp_config(num_mels, n_cep, unit_db, alarm_db, max_batch, max_frames)
        h = ctypes.c_void_p()
        rc = self.lib.wn_melcmp_create(ctypes.byref(self.cfg), ctypes.byref(h))
        if rc != 0:
            raise WnError(rc, (self.lib.wn_melcmp_last_error(None) or b'').decode())
        self.h = h
        self.num_mels, self.n_cep, self.max_batch, self.max_frames = int(num_mels), int(n_cep), int(max_batch), int(max_frames)
        self.unit_db, self.alarm_db = float(self.cfg.unit_db), float(self.cfg.alarm_db)

    def _ok(self, rc):
        if rc != 0:
            raise WnError(rc, (self.lib.wn_melcmp_last_error(self.h) or b'').decode())

    def run(self, a, b, frames, a_channels_first=True, b_channels_first=True, per_frame=False):
        """a, b float32 on the device, each [B, num_mels, pitch] (channels_first) or [B, pitch, num_mels]; frames: B ints (host).  Returns a dict of
        device tensors: 'summary' float32 [B, 7] (the means of MELCMP_KINDS, then worst), 'marks' int32 [B, 2] (worst frame, alarmed frames) and, with
        per_frame, 'per_frame' float32 [B, 6, pitch of the longest row] (elements beyond a row's frames are zero)."""
        import torch
        _check(a, torch.float32, 'a'); _check(b, torch.float32, 'b')
        B, ap = _melcmp_geometry(a, a_channels_first, self.num_mels, 'a')
        B2, bp = _melcmp_geometry(b, b_channels_first, self.num_mels, 'b')
        fr = [int(f) for f in frames]
        if B2 != B or len(fr) != B:
            raise ValueError('a, b and frames must have one entry per row')
        op = max(fr + [0])
        pf = torch.zeros(B, 6, op, dtype=torch.float32, device=a.device) if per_frame else None
        sm = torch.zeros(B, 7, dtype=torch.float32, device=a.device)
        mk = torch.zeros(B, 2, dtype=torch.int32, device=a.device)
        self._ok(self.lib.wn_melcmp_run(self.h, _ptr(a), int(bool(a_channels_first)), ap, _ptr(b), int(bool(b_channels_first)), bp, (ctypes.c_int32 * B)(*fr), B,
                                        _ptr(pf), op, _ptr(sm), _ptr(mk), _stream()))
        res = {'summary': sm, 'marks': mk}
        if per_frame:
            res['per_frame'] = pf
        return res

    def close(self):
        if getattr(self, 'h', None):
            self.lib.wn_melcmp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- alignment check (csrc/wn_align.hip)
ALIGN_COLUMNS = ('frames_a', 'frames_b', 'n_path', 'total', 'mcd_dtw', 'stretch', 'deviation')      # summary[b][j]
ALIGN_STAGES = ('cep_a', 'cep_b', 'cost', 'dm')                                                       # wn_test_align_copy's `what`


def align_config(num_mels, n_cep=13, unit_db=1.0, band=0, max_batch=0, max_frames_a=0, max_frames_b=0):
    cfg = WnAlignConfig()
    cfg.abi_version = WN_ABI_VERSION
    cfg.num_mels, cfg.n_cep, cfg.unit_db, cfg.band = int(num_mels), int(n_cep), float(unit_db), int(band)
    cfg.max_batch, cfg.max_frames_a, cfg.max_frames_b = int(max_batch), int(max_frames_a), int(max_frames_b)
    return cfg


def _align_rows(frames_a, frames_b, B):
    fa, fb = [int(f) for f in frames_a], [int(f) for f in frames_b]
    if len(fa) != B or len(fb) != B:
        raise ValueError('frames_a and frames_b must have one entry per row')
    return fa, fb


def _align_outputs(B, fa, fb, xp_full, path_pitch=None, map_a_pitch=None, map_b_pitch=None):
    """The four outputs of a call, filled with -7 / NaN (cells beyond a row's extent keep that); xp_full(shape, value, kind) makes one."""
    pp = max([a + b - 1 for a, b in zip(fa, fb)] + [1]) if path_pitch is None else int(path_pitch)
    pa = max(fa + [1]) if map_a_pitch is None else int(map_a_pitch)
    pb = max(fb + [1]) if map_b_pitch is None else int(map_b_pitch)
    return xp_full((B, 2, pp), -7, 'i'), xp_full((B, pa), -7, 'i'), xp_full((B, pb), -7, 'i'), xp_full((B, len(ALIGN_COLUMNS)), float('nan'), 'f'), pp, pa, pb


def _np_full(shape, value, kind):
    return np.full(shape, value, np.int32 if kind == 'i' else np.float32)


def align_host(a, b, frames_a, frames_b, num_mels=None, n_cep=13, unit_db=1.0, band=0, a_channels_first=True, b_channels_first=True, stages=False,
               path_pitch=None, map_a_pitch=None, map_b_pitch=None):
    """wn_test_align_host: the alignment check on the host (no handle, no GPU), in the device's order.  a, b: numpy float32, each [B, num_mels, pitch]
    (channels_first) or [B, pitch, num_mels].  Returns a dict: path int32 [B, 2, path_pitch], map_ab int32 [B, map_a_pitch], map_ba int32 [B, map_b_pitch],
    summary float32 [B, 7] (ALIGN_COLUMNS) and, with stages, cep_a [B, Fa_max, n_cep], cep_b [B, Fb_max, n_cep], cost and dm [B, Fa_max, Fb_max]; cells
    beyond a row's extent keep the -7 / NaN they are created with."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    M = int(a.shape[1 if a_channels_first else 2]) if num_mels is None else int(num_mels)
    B, ap = _melcmp_geometry(a, a_channels_first, M, 'a')
    B2, bp = _melcmp_geometry(b, b_channels_first, M, 'b')
    if B2 != B:
        raise ValueError('a and b must have one entry per row')
    fa, fb = _align_rows(frames_a, frames_b, B)
    cfg = align_config(M, n_cep, unit_db, band)
    path, mab, mba, sm, pp, pa, pb = _align_outputs(B, fa, fb, _np_full, path_pitch, map_a_pitch, map_b_pitch)
    res = {'path': path, 'map_ab': mab, 'map_ba': mba, 'summary': sm}
    vp = ctypes.c_void_p
    st = [None] * 4
    if stages:
        na, nb = max(fa + [1]), max(fb + [1])
        for k, shape in enumerate(((B, na, int(n_cep)), (B, nb, int(n_cep)), (B, na, nb), (B, na, nb))):
            res[ALIGN_STAGES[k]] = np.full(shape, np.nan, np.float32)
            st[k] = res[ALIGN_STAGES[k]].ctypes.data_as(vp)
    rc = load_library().wn_test_align_host(ctypes.byref(cfg), a.ctypes.data_as(vp), int(bool(a_channels_first)), ap, b.ctypes.data_as(vp), int(bool(b_channels_first)), bp,
                                           (ctypes.c_int32 * max(B, 1))(*fa), (ctypes.c_int32 * max(B, 1))(*fb), B, path.ctypes.data_as(vp), pp, mab.ctypes.data_as(vp), pa,
                                           mba.ctypes.data_as(vp), pb, sm.ctypes.data_as(vp), *st)
    if rc != 0:
        raise WnError(rc, (load_library().wn_align_last_error(None) or b'').decode())
    return res


def align_dp_host(cost, frames_a, frames_b, band=0, return_dm=True):
    """wn_test_align_dp_host: recurrence, back-trace and outputs on a caller's cost matrix, numpy float32 [B, Fa_max, Fb_max].  Returns the dict of
    align_host, with dm float32 [B, Fa_max, Fb_max] when return_dm."""
    cost = np.ascontiguousarray(cost, dtype=np.float32)
    if cost.ndim != 3:
        raise ValueError('cost must be [B, Fa_max, Fb_max]')
    B = int(cost.shape[0])
    fa, fb = _align_rows(frames_a, frames_b, B)
    path, mab, mba, sm, pp, pa, pb = _align_outputs(B, fa, fb, _np_full)
    dm = np.full(cost.shape, np.nan, np.float32) if return_dm else None
    vp = ctypes.c_void_p
    rc = load_library().wn_test_align_dp_host(int(band), cost.ctypes.data_as(vp), int(cost.shape[1]), int(cost.shape[2]), (ctypes.c_int32 * max(B, 1))(*fa),
                                              (ctypes.c_int32 * max(B, 1))(*fb), B, path.ctypes.data_as(vp), pp, mab.ctypes.data_as(vp), pa, mba.ctypes.data_as(vp), pb,
                                              sm.ctypes.data_as(vp), dm.ctypes.data_as(vp) if return_dm else None)
    if rc != 0:
        raise WnError(rc, (load_library().wn_align_last_error(None) or b'').decode())
    res = {'path': path, 'map_ab': mab, 'map_ba': mba, 'summary': sm}
    if return_dm:
        res['dm'] = dm
    return res


class Aligner:
    """One wn_align: dynamic time warping of two mel-spectrograms over their cepstral distance on the current device (csrc/wn_align.hip), asynchronously.
    max_batch = 0 gives a validation-only handle (no device; every run is refused)."""

    def __init__(self, num_mels, max_batch, max_frames_a, max_frames_b, n_cep=13, unit_db=1.0, band=0):
        self.lib = load_library()
        self.cfg = align_config(num_mels, n_cep, unit_db, band, max_batch, max_frames_a, max_frames_b)
        h = ctypes.c_void_p()
        rc = self.lib.wn_align_create(ctypes.byref(self.cfg), ctypes.byref(h))
        if rc != 0:
            raise WnError(rc, (self.lib.wn_align_last_error(None) or b'').decode())
        self.h = h
        self.num_mels, self.n_cep, self.band = int(num_mels), int(n_cep), int(band)
        self.max_batch, self.max_frames_a, self.max_frames_b = int(max_batch), int(max_frames_a), int(max_frames_b)

    def _ok(self, rc):
        if rc != 0:
            raise WnError(rc, (self.lib.wn_align_last_error(self.h) or b'').decode())

    @property
    def tile(self):
        return int(self.lib.wn_align_tile(self.h))

    def _outputs(self, B, fa, fb, device, want, out, pitches):
        import torch

        def full(shape, value, kind):
            return torch.full(shape, value, dtype=torch.int32 if kind == 'i' else torch.float32, device=device)
        if out is None:
            path, mab, mba, sm, _, _, _ = _align_outputs(B, fa, fb, full, *pitches)
            out = {'path': path, 'map_ab': mab, 'map_ba': mba, 'summary': sm}
            for k in ('path', 'map_ab', 'map_ba'):
                if k not in want:
                    out[k] = None
        for k in ('path', 'map_ab', 'map_ba'):
            if out.get(k) is not None:
                _check(out[k], torch.int32, k)
        _check(out['summary'], torch.float32, 'summary')
        if tuple(out['summary'].shape) != (B, len(ALIGN_COLUMNS)):
            raise ValueError('summary must be %r' % ((B, len(ALIGN_COLUMNS)),))

        def pitch(t, dim):
            if t is None:
                return 0
            if t.dim() != dim or int(t.shape[0]) != B or (dim == 3 and int(t.shape[1]) != 2):
                raise ValueError('an output of the wrong shape: %r' % (tuple(t.shape),))
            return int(t.shape[-1])
        return out, pitch(out.get('path'), 3), pitch(out.get('map_ab'), 2), pitch(out.get('map_ba'), 2)

    def run(self, a, b, frames_a, frames_b, a_channels_first=True, b_channels_first=True, want=('path', 'map_ab', 'map_ba'), out=None, pitches=(None, None, None)):
        """a, b float32 on the device, each [B, num_mels, pitch] (channels_first) or [B, pitch, num_mels]; frames_a, frames_b: B ints each (host).  Returns a
        dict of device tensors: 'summary' float32 [B, 7] (ALIGN_COLUMNS) and, as `want` lists them (None otherwise), 'path' int32 [B, 2, path_pitch],
        'map_ab' int32 [B, map_a_pitch], 'map_ba' int32 [B, map_b_pitch]; cells beyond a row's extent keep the -7 / NaN fresh tensors are created with.
        out: such a dict of ready tensors to write into instead; pitches: (path, map_a, map_b) pitches of fresh tensors."""
        import torch
        _check(a, torch.float32, 'a'); _check(b, torch.float32, 'b')
        B, ap = _melcmp_geometry(a, a_channels_first, self.num_mels, 'a')
        B2, bp = _melcmp_geometry(b, b_channels_first, self.num_mels, 'b')
        if B2 != B:
            raise ValueError('a and b must have one entry per row')
        fa, fb = _align_rows(frames_a, frames_b, B)
        out, pp, pa, pb = self._outputs(B, fa, fb, a.device, want, out, pitches)
        self._ok(self.lib.wn_align_run(self.h, _ptr(a), int(bool(a_channels_first)), ap, _ptr(b), int(bool(b_channels_first)), bp, (ctypes.c_int32 * B)(*fa),
                                       (ctypes.c_int32 * B)(*fb), B, _ptr(out.get('path')), pp, _ptr(out.get('map_ab')), pa, _ptr(out.get('map_ba')), pb, _ptr(out['summary']),
                                       _stream()))
        return out

    def run_dp(self, cost, frames_a, frames_b, want=('path', 'map_ab', 'map_ba'), out=None):
        """wn_test_align_dp: recurrence and back-trace on a caller's cost matrix, float32 [B, Fa_max, Fb_max] on the device; returns as run."""
        import torch
        _check(cost, torch.float32, 'cost')
        if cost.dim() != 3:
            raise ValueError('cost must be [B, Fa_max, Fb_max]')
        B = int(cost.shape[0])
        fa, fb = _align_rows(frames_a, frames_b, B)
        out, pp, pa, pb = self._outputs(B, fa, fb, cost.device, want, out, (None, None, None))
        self._ok(self.lib.wn_test_align_dp(self.h, _ptr(cost), int(cost.shape[1]), int(cost.shape[2]), (ctypes.c_int32 * B)(*fa), (ctypes.c_int32 * B)(*fb), B,
                                           _ptr(out.get('path')), pp, _ptr(out.get('map_ab')), pa, _ptr(out.get('map_ba')), pb, _ptr(out['summary']), _stream()))
        return out

    def store_matrix(self, on=True):
        self._ok(self.lib.wn_test_align_store_matrix(self.h, int(bool(on))))

    def copy_stage(self, what):
        """wn_test_align_copy (synchronises): the handle's own scratch of the last run as numpy float32 -- 'cep_a' [max_batch, max_frames_a, n_cep], 'cep_b'
        [max_batch, max_frames_b, n_cep], 'cost' or 'dm' [max_batch, max_frames_a, max_frames_b]."""
        k = ALIGN_STAGES.index(what)
        shape = ((self.max_batch, self.max_frames_a, self.n_cep), (self.max_batch, self.max_frames_b, self.n_cep), (self.max_batch, self.max_frames_a, self.max_frames_b),
                 (self.max_batch, self.max_frames_a, self.max_frames_b))[k]
        dst = np.empty(shape, np.float32)
        self._ok(self.lib.wn_test_align_copy(self.h, k, dst.ctypes.data_as(ctypes.c_void_p), int(dst.size), _stream()))
        return dst

    def close(self):
        if getattr(self, 'h', None):
            self.lib.wn_align_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- pitch check (csrc/wn_pitch.hip)
PITCH_COLUMNS = ('frames', 'voiced_a', 'voiced_b', 'both', 'vuv_error', 'gpe', 'f0_rmse_cents', 'f0_bias_cents', 'f0_fine_rmse_cents')      # table[b][j]
PITCH_GEOMETRY = ('sample_rate', 'hop', 'window', 'tau_min', 'tau_max', 'threshold')


def pitch_geometry(hp):
    """hparams -> the estimator's geometry: the mel analysis' hop, the lags of mi355_pitch_fmax ... mi355_pitch_fmin, window and threshold as given."""
    import math
    from datasets.audio import get_hop_size
    sr = int(hp.sample_rate)
    return dict(sample_rate=sr, hop=int(get_hop_size(hp)), window=int(getattr(hp, 'mi355_pitch_window', 1024)),
                tau_min=max(2, sr // int(float(getattr(hp, 'mi355_pitch_fmax', 500.0)))), tau_max=int(math.ceil(sr / float(getattr(hp, 'mi355_pitch_fmin', 60.0)))),
                threshold=float(getattr(hp, 'mi355_pitch_threshold', 0.15)))


def pitch_config(spec, max_batch, max_samples):
    """wn_pitch_config.  spec: hparams, or a dict with the keys PITCH_GEOMETRY."""
    geo = dict(spec) if isinstance(spec, dict) else pitch_geometry(spec)
    if set(geo) != set(PITCH_GEOMETRY):
        raise ValueError('pitch geometry must have exactly the keys %r (got %r)' % (PITCH_GEOMETRY, sorted(geo)))
    cfg = WnPitchConfig()
    cfg.abi_version = WN_ABI_VERSION
    for k in PITCH_GEOMETRY[:5]:
        setattr(cfg, k, int(geo[k]))
    cfg.threshold = float(geo['threshold'])
    cfg.max_batch, cfg.max_samples = int(max_batch), int(max_samples)
    return cfg


def _pitch_rows(wav, lengths):
    if wav.ndim != 2:
        raise ValueError('wav must be [B, ld]')
    lens = [int(n) for n in lengths]
    if len(lens) != int(wav.shape[0]):
        raise ValueError('one length per row of wav (%d lengths for %d rows)' % (len(lens), int(wav.shape[0])))
    return lens


def pitch_host(spec, wav, lengths, frames=None, return_dprime=False, fill=np.nan):
    """wn_test_pitch_host: the estimator on the host (no handle, no GPU), in the device's order.  wav: numpy float32 [B, ld].  Returns a dict: f0 and ap
    float32 [B, F_max] (F_max = frames or the frames of the longest row) and, with return_dprime, dprime float32 [B, F_max, tau_max + 1]; cells of frames
    beyond a row's keep `fill`."""
    wav = np.ascontiguousarray(wav, dtype=np.float32)
    lens = _pitch_rows(wav, lengths)
    B = len(lens)
    cfg = pitch_config(spec, max(B, 1), max(lens + [0]))
    F = int(frames) if frames is not None else max([1 + max(n, 0) // max(cfg.hop, 1) for n in lens] + [1])
    cfg.max_samples = max(int(cfg.max_samples), (F - 1) * max(int(cfg.hop), 1))          # the hook's capacity is the call's own: any F_max >= the rows' frames is taken
    f0, ap = np.full((B, F), fill, np.float32), np.full((B, F), fill, np.float32)
    dp = np.full((B, F, cfg.tau_max + 1), fill, np.float32) if return_dprime else None
    vp = ctypes.c_void_p
    rc = load_library().wn_test_pitch_host(ctypes.byref(cfg), wav.ctypes.data_as(vp), int(wav.shape[1]), (ctypes.c_int32 * max(B, 1))(*lens), B, F, f0.ctypes.data_as(vp),
                                           ap.ctypes.data_as(vp), dp.ctypes.data_as(vp) if return_dprime else None)
    if rc != 0:
        raise WnError(rc, (load_library().wn_pitch_last_error(None) or b'').decode())
    res = {'f0': f0, 'ap': ap}
    if return_dprime:
        res['dprime'] = dp
    return res


def pitch_compare_host(f0_a, f0_b, frames):
    """wn_test_pitch_compare_host: reference track a against generated track b, numpy float32 [B, pitch] each -> float32 [B, 9], columns PITCH_COLUMNS."""
    a, b = np.ascontiguousarray(f0_a, dtype=np.float32), np.ascontiguousarray(f0_b, dtype=np.float32)
    fr = [int(f) for f in frames]
    if a.ndim != 2 or a.shape != b.shape or len(fr) != int(a.shape[0]):
        raise ValueError('f0_a and f0_b must be [B, pitch] alike, with one frame count per row')
    B = len(fr)
    table = np.full((B, len(PITCH_COLUMNS)), np.nan, np.float32)
    vp = ctypes.c_void_p
    rc = load_library().wn_test_pitch_compare_host(a.ctypes.data_as(vp), b.ctypes.data_as(vp), int(a.shape[1]), (ctypes.c_int32 * max(B, 1))(*fr), B, table.ctypes.data_as(vp))
    if rc != 0:
        raise WnError(rc, (load_library().wn_pitch_last_error(None) or b'').decode())
    return table


class PitchTracker:
    """One wn_pitch: F0 and voicing per mel-aligned frame of a ragged batch on the current device (csrc/wn_pitch.hip), and the comparison of two tracks,
    asynchronously.  spec: hparams (pitch_geometry) or a dict with the keys PITCH_GEOMETRY."""

    def __init__(self, spec, rows, max_samples):
        self.lib = load_library()
        self.cfg = pitch_config(spec, rows, max_samples)
        h = ctypes.c_void_p()
        rc = self.lib.wn_pitch_create(ctypes.byref(self.cfg), ctypes.byref(h))
        if rc != 0:
            raise WnError(rc, (self.lib.wn_pitch_last_error(None) or b'').decode())
        self.h = h
        self.rows, self.max_samples = int(rows), int(max_samples)
        self.hop, self.tau_max, self.sample_rate = int(self.cfg.hop), int(self.cfg.tau_max), int(self.cfg.sample_rate)

    def _ok(self, rc):
        if rc != 0:
            raise WnError(rc, (self.lib.wn_pitch_last_error(self.h) or b'').decode())

    def num_frames(self, n):
        r = int(self.lib.wn_pitch_num_frames(self.h, int(n)))
        if r < 0:
            raise WnError(r, 'wn_pitch_num_frames(%d)' % n)
        return r

    @property
    def frame_tile(self):
        return int(self.lib.wn_pitch_frame_tile(self.h))

    def run(self, wav, lengths, return_dprime=False, frames=None, out=None):
        """wav float32 [B, ld] on the device, lengths: B ints (host).  Returns (f0, ap), float32 [B, F_max] each on the device (F_max = frames or the
        frames of the longest row), and with return_dprime also dprime float32 [B, F_max, tau_max + 1].  out: a tuple of ready tensors to write into
        instead (cells of frames beyond a row's keep their bytes; fresh tensors are zero there)."""
        import torch
        _check(wav, torch.float32, 'wav')
        lens = _pitch_rows(wav, lengths)
        B = len(lens)
        F = int(frames) if frames is not None else max(1 + n // self.hop for n in lens)
        if out is None:
            out = (torch.zeros(B, F, dtype=torch.float32, device=wav.device), torch.zeros(B, F, dtype=torch.float32, device=wav.device)) + (
                (torch.zeros(B, F, self.tau_max + 1, dtype=torch.float32, device=wav.device),) if return_dprime else ())
        shapes = [(B, F), (B, F)] + ([(B, F, self.tau_max + 1)] if return_dprime else [])
        if len(out) != len(shapes):
            raise ValueError('out must hold %d tensors' % len(shapes))
        for t, s in zip(out, shapes):
            _check(t, torch.float32, 'out')
            if tuple(t.shape) != s:
                raise ValueError('out must be %r (got %r)' % (s, tuple(t.shape)))
        self._ok(self.lib.wn_pitch_run(self.h, _ptr(wav), int(wav.shape[1]), (ctypes.c_int32 * B)(*lens), B, F, _ptr(out[0]), _ptr(out[1]),
                                       _ptr(out[2]) if return_dprime else None, _stream()))
        return tuple(out)

    def compare(self, f0_a, f0_b, frames, out=None):
        """Reference track f0_a against generated track f0_b, float32 [B, pitch] each on the device; frames: B ints (host) -> float32 [B, 9] on the
        device, columns PITCH_COLUMNS."""
        import torch
        _check(f0_a, torch.float32, 'f0_a'); _check(f0_b, torch.float32, 'f0_b')
        fr = [int(f) for f in frames]
        if f0_a.dim() != 2 or tuple(f0_a.shape) != tuple(f0_b.shape) or len(fr) != int(f0_a.shape[0]):
            raise ValueError('f0_a and f0_b must be [B, pitch] alike, with one frame count per row')
        B = len(fr)
        if out is None:
            out = torch.zeros(B, len(PITCH_COLUMNS), dtype=torch.float32, device=f0_a.device)
        _check(out, torch.float32, 'out')
        if tuple(out.shape) != (B, len(PITCH_COLUMNS)):
            raise ValueError('out must be %r' % ((B, len(PITCH_COLUMNS)),))
        self._ok(self.lib.wn_pitch_compare(self.h, _ptr(f0_a), _ptr(f0_b), int(f0_a.shape[1]), (ctypes.c_int32 * B)(*fr), B, _ptr(out), _stream()))
        return out

    def close(self):
        if getattr(self, 'h', None):
            self.lib.wn_pitch_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- spectral denoiser (csrc/wn_denoise.hip)
def denoise_config(n_fft, hop, max_batch=0, max_samples=0):
    cfg = WnDenoiseConfig()
    cfg.abi_version = WN_ABI_VERSION
    cfg.n_fft, cfg.hop, cfg.max_batch, cfg.max_samples = int(n_fft), int(hop), int(max_batch), int(max_samples)
    return cfg


def denoise_geometry(hp):
    """hparams -> (n_fft, hop) of the output denoiser (mi355_output_denoise_fft / mi355_output_denoise_hop)."""
    return int(getattr(hp, 'mi355_output_denoise_fft', 1024)), int(getattr(hp, 'mi355_output_denoise_hop', 256))


def denoise_host(n_fft, hop, wav=None, lengths=None, strength=0.0, profile=None, fit_wav=None, fit_lengths=None):
    """wn_test_denoise_host: fit and / or run in plain C++ float32 on numpy arrays (no handle, no GPU).  fit_wav [B', ld'] with fit_lengths: the profile is
    fitted from it, else `profile` [1 + n_fft / 2] is used.  wav [B, ld] with lengths: returns (out, profile), out a copy of wav with the first lengths[b]
    samples of every row denoised; wav None: returns (None, profile)."""
    vp = ctypes.c_void_p
    cfg = denoise_config(n_fft, hop)
    nb = 1 + max(int(n_fft), 0) // 2
    fw = fl = None
    fB = fld = 0
    if fit_wav is not None:
        fw = np.ascontiguousarray(fit_wav, dtype=np.float32)
        fls = _pitch_rows(fw, fit_lengths)
        fB, fld = len(fls), int(fw.shape[1])
        fl = (ctypes.c_int32 * max(fB, 1))(*fls)
        prof = np.zeros(nb, np.float32)
    else:
        prof = np.ascontiguousarray(profile, dtype=np.float32).copy()
        if prof.shape != (nb,):
            raise ValueError('profile must be [%d] (got %r)' % (nb, prof.shape))
    out = x = ln = None
    B = ld = 0
    if wav is not None:
        x = np.ascontiguousarray(wav, dtype=np.float32)
        lens = _pitch_rows(x, lengths)
        B, ld = len(lens), int(x.shape[1])
        ln = (ctypes.c_int32 * max(B, 1))(*lens)
        out = x.copy()
    rc = load_library().wn_test_denoise_host(ctypes.byref(cfg), None if fw is None else fw.ctypes.data_as(vp), fld, fl, fB, prof.ctypes.data_as(vp),
                                             None if x is None else x.ctypes.data_as(vp), ld, ln, B, float(strength), None if out is None else out.ctypes.data_as(vp), ld)
    if rc != 0:
        raise WnError(rc, (load_library().wn_denoise_last_error(None) or b'').decode())
    return out, prof


class SpectralDenoiser:
    """One wn_denoise: the bias denoiser on a ragged batch of decoded float signals on the current device (csrc/wn_denoise.hip), asynchronously: STFT
    (periodic Hann of n_fft at hop), every bin's magnitude lowered by strength x profile and clamped at zero with the phase kept, inverse transform and
    overlap-add.  The profile is fitted on the device (fit) or set from numpy (profile).  rows = 0: a geometry-only handle (validation, num_frames)."""

    def __init__(self, n_fft, hop, rows, max_samples):
        self.lib = load_library()
        self.cfg = denoise_config(n_fft, hop, rows, max_samples)
        h = ctypes.c_void_p()
        rc = self.lib.wn_denoise_create(ctypes.byref(self.cfg), ctypes.byref(h))
        if rc != 0:
            raise WnError(rc, (self.lib.wn_denoise_last_error(None) or b'').decode())
        self.h = h
        self.n_fft, self.hop, self.rows, self.max_samples = int(n_fft), int(hop), int(rows), int(max_samples)
        self.bins = 1 + self.n_fft // 2

    def _ok(self, rc):
        if rc != 0:
            raise WnError(rc, (self.lib.wn_denoise_last_error(self.h) or b'').decode())

    def num_frames(self, n):
        r = int(self.lib.wn_denoise_num_frames(self.h, int(n)))
        if r < 0:
            raise WnError(r, 'wn_denoise_num_frames(%d)' % n)
        return r

    def fit(self, wav, lengths):
        """wav float32 [B, ld] on the device, lengths: B ints (host): the handle's profile becomes the mean magnitude of the frames wholly inside the rows."""
        import torch
        _check(wav, torch.float32, 'wav')
        lens = _pitch_rows(wav, lengths)
        self._ok(self.lib.wn_denoise_fit(self.h, _ptr(wav), int(wav.shape[1]), (ctypes.c_int32 * max(len(lens), 1))(*lens), len(lens), _stream()))

    @property
    def profile(self):
        """The profile as numpy float32 [1 + n_fft / 2] (synchronises the current stream)."""
        p = np.zeros(self.bins, np.float32)
        self._ok(self.lib.wn_denoise_get_profile(self.h, p.ctypes.data_as(ctypes.c_void_p), _stream() if self.rows > 0 else None))
        return p

    @profile.setter
    def profile(self, value):
        p = np.ascontiguousarray(value, dtype=np.float32)
        if p.shape != (self.bins,):
            raise ValueError('profile must be [%d] (got %r)' % (self.bins, p.shape))
        self._ok(self.lib.wn_denoise_set_profile(self.h, p.ctypes.data_as(ctypes.c_void_p), _stream() if self.rows > 0 else None))

    def apply(self, wav, lengths, strength, out=None):
        """wav float32 [B, ld] on the device -> out (fresh: a copy of wav; out=wav: in place) with the first lengths[b] samples of row b denoised at
        `strength`; what lies beyond keeps its bytes."""
        import torch
        _check(wav, torch.float32, 'wav')
        lens = _pitch_rows(wav, lengths)
        if out is None:
            out = wav.clone()
        _check(out, torch.float32, 'out')
        if out.dim() != 2 or int(out.shape[0]) != len(lens):
            raise ValueError('out must be [B, pitch] with one row per row of wav')
        self._ok(self.lib.wn_denoise_run(self.h, _ptr(wav), int(wav.shape[1]), (ctypes.c_int32 * max(len(lens), 1))(*lens), len(lens), float(strength), _ptr(out),
                                         int(out.shape[1]), _stream()))
        return out

    def close(self):
        if getattr(self, 'h', None):
            self.lib.wn_denoise_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- Griffin-Lim baseline (csrc/wn_griffin.hip)
GRIFFIN_SRC = {'mel': 0, 'mel_cf': 1, 'magnitude': 2}
GRIFFIN_CONTINUE = 1


def griffin_config(n_fft, win_size, hop, num_mels=0, magnitude_power=1.0, power=1.0, min_level_db=-100.0, ref_level_db=0.0, max_abs_value=1.0,
                   signal_normalization=False, allow_clipping=False, symmetric_mels=False, max_batch=0, max_frames=0):
    cfg = WnGriffinConfig()
    cfg.abi_version = WN_ABI_VERSION
    cfg.n_fft, cfg.win_size, cfg.hop, cfg.num_mels = int(n_fft), int(win_size), int(hop), int(num_mels)
    cfg.magnitude_power, cfg.power = float(magnitude_power), float(power)
    cfg.min_level_db, cfg.ref_level_db, cfg.max_abs_value = float(min_level_db), float(ref_level_db), float(max_abs_value)
    cfg.signal_normalization, cfg.allow_clipping, cfg.symmetric_mels = int(bool(signal_normalization)), int(bool(allow_clipping)), int(bool(symmetric_mels))
    cfg.max_batch, cfg.max_frames = int(max_batch), int(max_frames)
    return cfg


def griffin_config_from_hparams(hp, max_batch=0, max_frames=0):
    """hparams (reference keys, hparams.py:102-133, 150-152) -> wn_griffin_config"""
    from datasets.audio import get_hop_size
    return griffin_config(hp.n_fft, hp.n_fft if hp.win_size is None else hp.win_size, get_hop_size(hp), hp.num_mels, hp.magnitude_power, hp.power,
                          hp.min_level_db, hp.ref_level_db, hp.max_abs_value, hp.signal_normalization, hp.allow_clipping_in_normalization, hp.symmetric_mels,
                          max_batch, max_frames)


def griffin_pinv(hp):
    """np.linalg.pinv(mel_basis) in float64, rounded to float32 once: [1 + n_fft / 2, num_mels] (reference audio.py:231-235)"""
    from datasets.audio import _build_mel_basis
    return np.ascontiguousarray(np.linalg.pinv(np.asarray(_build_mel_basis(hp), np.float64)).astype(np.float32))


def _griffin_src(cfg, src, kind, frames):
    """(kind code, B, F_max, frames array) of a source array [B, F_max, num_mels] ('mel'), [B, num_mels, F_max] ('mel_cf') or [B, F_max, bins] ('magnitude')"""
    if kind not in GRIFFIN_SRC:
        raise ValueError("kind must be 'mel', 'mel_cf' or 'magnitude' (got %r)" % (kind,))
    if src.ndim != 3:
        raise ValueError('the source must have three dimensions')
    B = int(src.shape[0])
    width = 1 + int(cfg.n_fft) // 2 if kind == 'magnitude' else int(cfg.num_mels)
    F_max = int(src.shape[2] if kind == 'mel_cf' else src.shape[1])
    if int(src.shape[1] if kind == 'mel_cf' else src.shape[2]) != width:
        raise ValueError('the source of kind %r must have %d channels (got shape %r)' % (kind, width, tuple(src.shape)))
    if len(frames) != B:
        raise ValueError('one frame count per row (%d for %d rows)' % (len(frames), B))
    return GRIFFIN_SRC[kind], B, F_max, (ctypes.c_int32 * max(B, 1))(*[int(f) for f in frames])


def griffin_host(cfg, src, frames, kind='magnitude', pinv=None, u=None, y0=None, iters=0, return_all=False, fill=0.0):
    """wn_test_griffin_host: a run in plain C++ float32 on numpy arrays (no handle, no GPU).  Returns out [B, hop (F_max - 1)] (`fill` beyond a row's samples),
    with return_all also the magnitudes [B, F_max, bins] and the spectrum before the last projection, complex64 [B, F_max, bins]."""
    vp = ctypes.c_void_p
    src = np.ascontiguousarray(src, dtype=np.float32)
    code, B, F_max, fr = _griffin_src(cfg, src, kind, frames)
    nb = 1 + int(cfg.n_fft) // 2
    pitch = max(1, int(cfg.hop) * max(F_max - 1, 0))
    out = np.full((B, pitch), fill, np.float32)
    p = None if pinv is None else np.ascontiguousarray(pinv, dtype=np.float32)
    if p is not None and p.shape != (nb, int(cfg.num_mels)):
        raise ValueError('pinv must be [%d, %d] (got %r)' % (nb, int(cfg.num_mels), p.shape))
    uu = None if u is None else np.ascontiguousarray(u, dtype=np.float32)
    if uu is not None and uu.shape != (B, F_max, nb):
        raise ValueError('u must be [%d, %d, %d]' % (B, F_max, nb))
    yy = None if y0 is None else np.ascontiguousarray(y0, dtype=np.float32)
    mag = np.zeros((B, F_max, nb), np.float32)
    pre = np.zeros((B, F_max, nb, 2), np.float32)
    lib = load_library()
    rc = lib.wn_test_griffin_host(ctypes.byref(cfg), None if p is None else p.ctypes.data_as(vp), src.ctypes.data_as(vp), code, F_max, fr, B,
                                  None if uu is None else uu.ctypes.data_as(vp), None if yy is None else yy.ctypes.data_as(vp), 0 if yy is None else int(yy.shape[1]),
                                  int(iters), out.ctypes.data_as(vp), pitch, mag.ctypes.data_as(vp), pre.ctypes.data_as(vp))
    if rc != 0:
        raise WnError(rc, (lib.wn_griffin_last_error(None) or b'').decode())
    return (out, mag, pre[..., 0] + 1j * pre[..., 1]) if return_all else out


class GriffinLim:
    """One wn_griffin: normalised mels (or magnitudes) -> signals by Griffin-Lim on the current device (csrc/wn_griffin.hip), asynchronously: the reference's
    inv_mel_spectrogram up to the de-emphasis.  Built from hparams with pinv(mel_basis) computed in float64; rows = 0: a geometry-only handle."""

    def __init__(self, hparams, rows, max_frames, pinv=None, cfg=None):
        """cfg: a wn_griffin_config to use instead of the one hparams gives (tests; hparams may then be None); pinv [1 + n_fft / 2, num_mels]: default
        griffin_pinv(hparams), with cfg given: none (a handle that takes magnitudes only)."""
        if hparams is not None and getattr(hparams, 'use_lws', False):
            raise NotImplementedError('use_lws: the lws package is not available')
        self.lib = load_library()
        if cfg is None:
            cfg = griffin_config_from_hparams(hparams, rows, max_frames)
            if pinv is None and rows > 0:
                pinv = griffin_pinv(hparams)
        else:
            cfg.max_batch, cfg.max_frames = int(rows), int(max_frames)
        self.cfg = cfg
        self.bins = 1 + int(cfg.n_fft) // 2
        p = None
        if pinv is not None:
            p = np.ascontiguousarray(pinv, dtype=np.float32)
            if p.shape != (self.bins, int(cfg.num_mels)):
                raise ValueError('pinv must be [1 + n_fft // 2, num_mels] = %r (got %r)' % ((self.bins, int(cfg.num_mels)), p.shape))
        h = ctypes.c_void_p()
        rc = self.lib.wn_griffin_create(ctypes.byref(cfg), None if p is None else p.ctypes.data_as(ctypes.c_void_p), ctypes.byref(h))
        if rc != 0:
            raise WnError(rc, (self.lib.wn_griffin_last_error(None) or b'').decode())
        self.h = h
        self.hop, self.rows, self.max_frames = int(cfg.hop), int(rows), int(max_frames)
        self._frames = None

    def _ok(self, rc):
        if rc != 0:
            raise WnError(rc, (self.lib.wn_griffin_last_error(self.h) or b'').decode())

    def num_samples(self, frames):
        r = int(self.lib.wn_griffin_num_samples(self.h, int(frames)))
        if r < 0:
            raise WnError(r, 'wn_griffin_num_samples(%d)' % frames)
        return r

    def _out(self, out, B, frames, device):
        import torch
        if out is None:
            out = torch.zeros((B, max(1, self.hop * (max(frames) - 1))), dtype=torch.float32, device=device)
        _check(out, torch.float32, 'out')
        if out.dim() != 2 or int(out.shape[0]) != B:
            raise ValueError('out must be [B, pitch]')
        return out

    def _run(self, src, kind, frames, iters, u, y0, out, seed):
        import torch
        _check(src, torch.float32, 'src')
        code, B, F_max, fr = _griffin_src(self.cfg, src, kind, frames)
        if y0 is not None:
            _check(y0, torch.float32, 'y0')
            if y0.dim() != 2 or int(y0.shape[0]) != B:
                raise ValueError('y0 must be [B, pitch]')
        elif u is None and seed is not None:      # the reference's np.random.rand start, from a seeded torch generator on the device: no RNG of our own
            gen = torch.Generator(device=src.device)
            gen.manual_seed(int(seed))
            u = torch.rand((B, F_max, self.bins), dtype=torch.float32, device=src.device, generator=gen)
        if u is not None:
            _check(u, torch.float32, 'u')
            if tuple(u.shape) != (B, F_max, self.bins):
                raise ValueError('u must be %r' % ((B, F_max, self.bins),))
        out = self._out(out, B, [int(f) for f in frames], src.device)
        self._ok(self.lib.wn_griffin_run(self.h, _ptr(src), code, F_max, fr, B, _ptr(u), _ptr(y0), 0 if y0 is None else int(y0.shape[1]), int(iters), 0, _ptr(out),
                                         int(out.shape[1]), _stream()))
        self._frames = [int(f) for f in frames]
        return out

    def run_mel(self, mel, frames, iters=60, channels_first=False, u=None, y0=None, seed=0, out=None):
        """mel float32 [B, F_max, num_mels] (channels_first: [B, num_mels, F_max]) on the device, frames: B ints (host) -> out [B, pitch] on the device, row b
        holding hop (frames[b] - 1) samples (pre-emphasised domain).  The start: y0 if given, else the uniforms u [B, F_max, bins] if given, else uniforms drawn
        on the device from `seed` (seed None: zero phase); then `iters` iterations."""
        return self._run(mel, 'mel_cf' if channels_first else 'mel', frames, iters, u, y0, out, seed)

    def run_magnitude(self, S, frames, iters=60, u=None, y0=None, seed=0, out=None):
        """S float32 [B, F_max, 1 + n_fft / 2] on the device, used as is; otherwise as run_mel"""
        return self._run(S, 'magnitude', frames, iters, u, y0, out, seed)

    def continue_(self, iters, out=None):
        """`iters` further iterations on the rows of the last run -> out [B, pitch]: run(a) then continue_(b) has the bits of run(a + b)"""
        import torch
        if self._frames is None:
            raise WnError(-5, 'GriffinLim.continue_: no run has been made on this handle')
        out = self._out(out, len(self._frames), self._frames, torch.device('cuda', torch.cuda.current_device()))
        self._ok(self.lib.wn_griffin_run(self.h, None, 0, 0, None, 0, None, None, 0, int(iters), GRIFFIN_CONTINUE, _ptr(out), int(out.shape[1]), _stream()))
        return out

    # test hooks
    def store_spectrum(self, on=True):
        self._ok(self.lib.wn_test_griffin_store_spectrum(self.h, int(bool(on))))

    def magnitudes(self, F_max):
        """the magnitudes of the last run as numpy [B, F_max, bins] (synchronises)"""
        m = np.zeros((len(self._frames), int(F_max), self.bins), np.float32)
        self._ok(self.lib.wn_test_griffin_copy(self.h, 0, m.ctypes.data_as(ctypes.c_void_p), int(F_max), _stream()))
        return m

    def spectrum(self, F_max):
        """the spectrum before the last projection as numpy complex64 [B, F_max, bins] (store_spectrum must be on; synchronises)"""
        p = np.zeros((len(self._frames), int(F_max), self.bins, 2), np.float32)
        self._ok(self.lib.wn_test_griffin_copy(self.h, 1, p.ctypes.data_as(ctypes.c_void_p), int(F_max), _stream()))
        return p[..., 0] + 1j * p[..., 1]

    def close(self):
        if getattr(self, 'h', None):
            self.lib.wn_griffin_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- streaming spectral denoiser (csrc/wn_denoise_stream.hip)
def denoise_stream_config(n_fft, hop, max_rows=0, max_push=1, in_type=0):
    cfg = WnDenoiseStreamConfig()
    cfg.abi_version = WN_ABI_VERSION
    cfg.n_fft, cfg.hop, cfg.max_rows, cfg.max_push = int(n_fft), int(hop), int(max_rows), int(max_push)
    cfg.in_type = INPUT_TYPES[in_type] if in_type in INPUT_TYPES else int(in_type)
    return cfg


def denoise_stream_ready(n_fft, hop, S, final=False):
    """The emit rule in Python (what wn_denoise_stream_ready computes): samples emitted of a row that was given S since its restart."""
    S, H = int(S), int(n_fft) // 2
    if final:
        return S
    return max(0, ((S - H) // int(hop) + 1) * int(hop) - H)


def denoise_stream_host(n_fft, hop, pushes, profile, strength, in_type=0, max_push=None):
    """wn_test_denoise_stream_host: the streaming state machine in plain C++ float32 on numpy arrays (no handle, no GPU).  pushes: a list of
    (block [B, pitch] float32 / int32, n [B], restart [B] or None, final [B] or None).  Returns a list of (out [B, out_pitch] float32, n_out [B]) per push:
    out rows hold n_out[b] samples, what lies beyond keeps the fill it was given (`nan`)."""
    vp = ctypes.c_void_p
    P = len(pushes)
    B = len(pushes[0][1])
    dt = np.int32 if (INPUT_TYPES[in_type] if in_type in INPUT_TYPES else int(in_type)) == 2 else np.float32
    ipitch = max([1] + [int(np.asarray(p[0]).reshape(B, -1).shape[1]) for p in pushes])
    n = np.zeros((P, B), np.int32); rs = np.zeros((P, B), np.int32); fin = np.zeros((P, B), np.int32)
    blk = np.zeros((P, B, ipitch), dt)
    if dt == np.float32:
        blk[:] = np.nan
    for p, (x, nn, r, f) in enumerate(pushes):
        x = np.asarray(x, dtype=dt).reshape(B, -1)
        blk[p, :, :x.shape[1]] = x
        n[p] = nn
        if r is not None:
            rs[p] = np.asarray(r, np.int32)
        if f is not None:
            fin[p] = np.asarray(f, np.int32)
    cfg = denoise_stream_config(n_fft, hop, 0, max(1, int(n.max()) if max_push is None else int(max_push)), in_type)
    opitch = int(n.max()) + int(n_fft) + 3
    out = np.full((P, B, opitch), np.nan, np.float32)
    n_out = np.full((P, B), -1, np.int32)
    prof = np.ascontiguousarray(profile, dtype=np.float32)
    rc = load_library().wn_test_denoise_stream_host(ctypes.byref(cfg), prof.ctypes.data_as(vp), float(strength), blk.ctypes.data_as(vp), ipitch, n.ctypes.data_as(vp),
                                                    rs.ctypes.data_as(vp), fin.ctypes.data_as(vp), P, B, out.ctypes.data_as(vp), opitch, n_out.ctypes.data_as(vp))
    if rc != 0:
        raise WnError(rc, (load_library().wn_denoise_stream_last_error(None) or b'').decode())
    return [(out[p], n_out[p]) for p in range(P)]


class DenoiseStream:
    """One wn_denoise_stream: the spectral denoiser on rows that arrive push by push on the current device (csrc/wn_denoise_stream.hip), asynchronously.  A
    row's emitted samples, concatenated, are bit-identical to SpectralDenoiser.apply on the whole row; they lag the samples given by less than n_fft (ready()).
    rows = 0: a geometry-only handle.  Use one handle from one stream at a time."""

    def __init__(self, n_fft, hop, rows, max_push, in_type=0):
        self.lib = load_library()
        self.cfg = denoise_stream_config(n_fft, hop, rows, max_push, in_type)
        h = ctypes.c_void_p()
        rc = self.lib.wn_denoise_stream_create(ctypes.byref(self.cfg), ctypes.byref(h))
        if rc != 0:
            raise WnError(rc, (self.lib.wn_denoise_stream_last_error(None) or b'').decode())
        self.h = h
        self.n_fft, self.hop, self.rows, self.max_push, self.in_type = int(n_fft), int(hop), int(rows), int(max_push), int(self.cfg.in_type)
        self.bins = 1 + self.n_fft // 2

    def _ok(self, rc):
        if rc != 0:
            raise WnError(rc, (self.lib.wn_denoise_stream_last_error(self.h) or b'').decode())

    def ready(self, S, final=False):
        r = int(self.lib.wn_denoise_stream_ready(self.h, int(S), int(bool(final))))
        if r < 0:
            raise WnError(r, 'wn_denoise_stream_ready(%d)' % S)
        return r

    def set_profile(self, value):
        p = np.ascontiguousarray(value, dtype=np.float32)
        if p.shape != (self.bins,):
            raise ValueError('profile must be [%d] (got %r)' % (self.bins, p.shape))
        self._ok(self.lib.wn_denoise_stream_set_profile(self.h, p.ctypes.data_as(ctypes.c_void_p), _stream() if self.rows > 0 else None))

    def take_profile(self, source):
        """The fitted or set profile of a SpectralDenoiser of the same n_fft, device to device on the current stream (nothing synchronises)."""
        self._ok(self.lib.wn_denoise_stream_take_profile(self.h, source.h, _stream() if self.rows > 0 else None))

    def push(self, samples, n=None, restart=None, final=None, strength=0.0, out=None):
        """samples [B, pitch] on the device (float32, or int32 class ids with in_type 2), n: B ints (None: the whole pitch), restart / final: B flags
        (None: none; True: all).  Returns (out float32 [B, max(n) + n_fft] on the device, contiguous, n_out: B ints): row b's next n_out[b] denoised samples, zeros
        beyond.  out: a float32 [B, pitch'] tensor to write into instead (elements beyond n_out[b] keep their bytes)."""
        import torch
        _check(samples, torch.int32 if self.in_type == 2 else torch.float32, 'samples')
        if samples.dim() == 1:
            samples = samples.reshape(1, -1)
        if samples.dim() != 2:
            raise ValueError('samples must be [B, pitch]')
        B, pitch = int(samples.shape[0]), int(samples.shape[1])
        n = [pitch] * B if n is None else [int(v) for v in n]
        if len(n) != B:
            raise ValueError('one length per row of samples (%d lengths for %d rows)' % (len(n), B))

        def flags(v, name):
            if v is None:
                return None
            f = [1] * B if v is True else [int(bool(x)) for x in v]
            if len(f) != B:
                raise ValueError('one %s flag per row' % name)
            return (ctypes.c_int32 * B)(*f)
        rs, fin = flags(restart, 'restart'), flags(final, 'final')
        if out is None:
            out = torch.zeros(B, max(max(n), 0) + self.n_fft, dtype=torch.float32, device=samples.device)      # a push emits at most n + (S - E) < n + n_fft samples
        _check(out, torch.float32, 'out')
        if out.dim() != 2 or int(out.shape[0]) != B:
            raise ValueError('out must be [B, pitch] with one row per row of samples')
        opitch = int(out.shape[1])
        n_out = (ctypes.c_int32 * B)()
        self._ok(self.lib.wn_denoise_stream_push(self.h, _ptr(samples), pitch, (ctypes.c_int32 * B)(*n), rs, fin, B, float(strength), _ptr(out), opitch, n_out, _stream()))
        n_out = [int(v) for v in n_out]
        return out, n_out

    def close(self):
        if getattr(self, 'h', None):
            self.lib.wn_denoise_stream_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- sample-rate conversion (csrc/wn_resample.hip)
RESAMPLE_ZEROS, RESAMPLE_BETA, RESAMPLE_ROLLOFF = 64, 14.769656459379492, 0.9475937167399596      # resampy's published kaiser_best design values


def resample_config(sr_in, sr_out, max_rows=0, max_in=0, zeros=RESAMPLE_ZEROS, beta=RESAMPLE_BETA, rolloff=RESAMPLE_ROLLOFF):
    cfg = WnResampleConfig()
    cfg.abi_version = WN_ABI_VERSION
    cfg.max_rows, cfg.max_in, cfg.sr_in, cfg.sr_out, cfg.zeros = int(max_rows), int(max_in), int(sr_in), int(sr_out), int(zeros)
    cfg.beta, cfg.rolloff = float(beta), float(rolloff)
    return cfg


def resample_table(sr_in, sr_out, zeros=RESAMPLE_ZEROS, beta=RESAMPLE_BETA, rolloff=RESAMPLE_ROLLOFF):
    """wn_test_resample_table: the float32 coefficient table C [L, T] of a configuration, as the device holds it ([0, 0] for sr_in == sr_out)."""
    rs = Resampler(sr_in, sr_out, 0, 0, zeros, beta, rolloff)
    C = np.zeros((rs.L, 2 * rs.W), np.float32)
    rc = rs.lib.wn_test_resample_table(ctypes.byref(rs.cfg), C.ctypes.data_as(ctypes.c_void_p), C.size)
    if rc != 0:
        raise WnError(rc, (rs.lib.wn_resample_last_error(None) or b'').decode())
    return C


def resample_host(pushes, sr_in, sr_out, zeros=RESAMPLE_ZEROS, beta=RESAMPLE_BETA, rolloff=RESAMPLE_ROLLOFF, max_in=0):
    """wn_test_resample_host: the state machine of Resampler.push as a plain float32 loop on numpy arrays (no handle, no GPU), bit-identical to the device.
    pushes: a list of (block [B, pitch] float32, n [B], restart [B] or None, final [B] or None).  Returns a list of (out [B, out_pitch] float32, n_out [B]) per
    push: out rows hold n_out[b] samples, what lies beyond keeps the fill it was given (`nan`)."""
    vp = ctypes.c_void_p
    P = len(pushes)
    B = len(pushes[0][1])
    ipitch = max([1] + [int(np.asarray(p[0]).reshape(B, -1).shape[1]) for p in pushes])
    n = np.zeros((P, B), np.int32); rs = np.zeros((P, B), np.int32); fin = np.zeros((P, B), np.int32)
    blk = np.full((P, B, ipitch), np.nan, np.float32)
    for p, (x, nn, r, f) in enumerate(pushes):
        x = np.asarray(x, dtype=np.float32).reshape(B, -1)
        blk[p, :, :x.shape[1]] = x
        n[p] = nn
        if r is not None:
            rs[p] = np.asarray(r, np.int32)
        if f is not None:
            fin[p] = np.asarray(f, np.int32)
    cfg = resample_config(sr_in, sr_out, 0, max_in, zeros, beta, rolloff)
    lib = load_library()
    geo = Resampler(sr_in, sr_out, 0, max_in, zeros, beta, rolloff)
    opitch = geo.num_out(max(0, int(n.max())) + 2 * geo.W) + 3      # a push emits the outputs of at most n + 2 W - 1 inputs
    out = np.full((P, B, opitch), np.nan, np.float32)
    n_out = np.full((P, B), -1, np.int32)
    rc = lib.wn_test_resample_host(ctypes.byref(cfg), blk.ctypes.data_as(vp), ipitch, n.ctypes.data_as(vp), rs.ctypes.data_as(vp), fin.ctypes.data_as(vp), P, B,
                                   out.ctypes.data_as(vp), opitch, n_out.ctypes.data_as(vp))
    if rc != 0:
        raise WnError(rc, (lib.wn_resample_last_error(None) or b'').decode())
    return [(out[p], n_out[p]) for p in range(P)]


def resample_rows_host(rows, sr_in, sr_out, zeros=RESAMPLE_ZEROS, beta=RESAMPLE_BETA, rolloff=RESAMPLE_ROLLOFF):
    """Whole rows through wn_test_resample_host (one final push): a list of 1-D float32 arrays in, a list of float32 arrays of ceil(n L / M) samples out."""
    rows = [np.ascontiguousarray(r, dtype=np.float32).reshape(-1) for r in rows]
    blk = np.zeros((len(rows), max([1] + [len(r) for r in rows])), np.float32)
    for b, r in enumerate(rows):
        blk[b, :len(r)] = r
    (out, n_out), = resample_host([(blk, [len(r) for r in rows], None, [1] * len(rows))], sr_in, sr_out, zeros, beta, rolloff)
    return [out[b, :n_out[b]].copy() for b in range(len(rows))]


class Resampler:
    """One wn_resample: rows of float32 samples from sr_in to sr_out on the current device (csrc/wn_resample.hip), asynchronously: whole ragged rows (run) or
    push by push with carried state (push; row = slot).  A row's pushed outputs, concatenated, are bit-identical to run on the whole row and to resample_host;
    they lag the inputs by at most W samples (ready()).  rows = 0: a geometry-only handle (num_out, ready, L / M / W) that needs no GPU.  Use one handle from one
    stream at a time."""

    def __init__(self, sr_in, sr_out, rows, max_in, zeros=RESAMPLE_ZEROS, beta=RESAMPLE_BETA, rolloff=RESAMPLE_ROLLOFF):
        self.lib = load_library()
        self.cfg = resample_config(sr_in, sr_out, rows, max_in, zeros, beta, rolloff)
        h = ctypes.c_void_p()
        rc = self.lib.wn_resample_create(ctypes.byref(self.cfg), ctypes.byref(h))
        if rc != 0:
            raise WnError(rc, (self.lib.wn_resample_last_error(None) or b'').decode())
        self.h = h
        self.sr_in, self.sr_out, self.rows, self.max_in = int(sr_in), int(sr_out), int(rows), int(max_in)
        L, M, W = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        self._ok(self.lib.wn_resample_taps(self.h, ctypes.byref(L), ctypes.byref(M), ctypes.byref(W)))
        self.L, self.M, self.W = int(L.value), int(M.value), int(W.value)

    def _ok(self, rc):
        if rc != 0:
            raise WnError(rc, (self.lib.wn_resample_last_error(self.h) or b'').decode())

    def num_out(self, n):
        r = int(self.lib.wn_resample_num_out(self.h, int(n)))
        if r < 0:
            raise WnError(r, 'wn_resample_num_out(%d)' % n)
        return r

    def ready(self, S, final=False):
        r = int(self.lib.wn_resample_ready(self.h, int(S), int(bool(final))))
        if r < 0:
            raise WnError(r, 'wn_resample_ready(%d)' % S)
        return r

    @staticmethod
    def _rows(samples, n, what):
        import torch
        _check(samples, torch.float32, 'samples')
        if samples.dim() == 1:
            samples = samples.reshape(1, -1)
        if samples.dim() != 2:
            raise ValueError('samples must be [B, pitch]')
        B, pitch = int(samples.shape[0]), int(samples.shape[1])
        n = [pitch] * B if n is None else [int(v) for v in n]
        if len(n) != B:
            raise ValueError('one %s per row of samples (%d for %d rows)' % (what, len(n), B))
        return samples, n, B, pitch

    @staticmethod
    def _out(out, B):
        import torch
        _check(out, torch.float32, 'out')
        if out.dim() != 2 or int(out.shape[0]) != B:
            raise ValueError('out must be [B, pitch] with one row per row of samples')
        return int(out.shape[1])

    def run(self, samples, lengths=None, out=None):
        """samples [B, pitch] float32 on the device, lengths: B ints (None: the whole pitch).  Returns (out float32 [B, num_out(max(lengths))] on the device,
        n_out: B ints): row b holds num_out(lengths[b]) samples, zeros beyond.  out: a float32 [B, pitch'] tensor to write into instead (elements beyond a
        row's outputs keep their bytes).  Carried state is neither read nor written."""
        import torch
        samples, n, B, pitch = self._rows(samples, lengths, 'length')
        if out is None:
            out = torch.zeros(B, max(1, self.num_out(max(max(n), 0))), dtype=torch.float32, device=samples.device)
        opitch = self._out(out, B)
        self._ok(self.lib.wn_resample_run(self.h, _ptr(samples), pitch, (ctypes.c_int32 * B)(*n), B, _ptr(out), opitch, _stream()))
        return out, [self.num_out(v) for v in n]

    def push(self, samples, n=None, restart=None, final=None, out=None):
        """samples [B, pitch] float32 on the device, n: B ints (None: the whole pitch), restart / final: B flags (None: none; True: all).  Returns (out float32
        [B, pitch'] on the device, n_out: B ints): row b's next n_out[b] samples at sr_out, zeros beyond (with out given: its bytes kept)."""
        import torch
        samples, n, B, pitch = self._rows(samples, n, 'count')

        def flags(v, name):
            if v is None:
                return None
            f = [1] * B if v is True else [int(bool(x)) for x in v]
            if len(f) != B:
                raise ValueError('one %s flag per row' % name)
            return (ctypes.c_int32 * B)(*f)
        rs, fin = flags(restart, 'restart'), flags(final, 'final')
        if out is None:
            out = torch.zeros(B, self.num_out(max(max(n), 0) + 2 * self.W) + 1, dtype=torch.float32, device=samples.device)      # a push emits the outputs of at most n + 2 W - 1 inputs
        opitch = self._out(out, B)
        n_out = (ctypes.c_int32 * B)()
        self._ok(self.lib.wn_resample_push(self.h, _ptr(samples), pitch, (ctypes.c_int32 * B)(*n), rs, fin, B, _ptr(out), opitch, n_out, _stream()))
        return out, [int(v) for v in n_out]

    def close(self):
        if getattr(self, 'h', None):
            self.lib.wn_resample_destroy(self.h)
            self.h = None
        if getattr(self, 'tail', None) is not None:      # (WaveNet.output_resampler's int16 stage)
            self.tail.close()
            self.tail = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- training summaries (csrc/wn_stats.hip)
WN_HIST_BUCKETS = 1551
HIST_SUMMARY = ('num', 'min', 'max', 'sum', 'sum_squares', 'n_nan', 'n_pos_inf', 'n_neg_inf')      # summary[8] of a histogram
TENSOR_STATS = ('sum_squares', 'max_abs', 'nonfinite', 'count')                                     # out[t][4] of the per-tensor statistics
_hist_limits = None


def hist_limits():
    """wn_stats_hist_limits: the WN_HIST_BUCKETS ascending bucket limits (TensorFlow's default summary table) as float64.  Host only."""
    global _hist_limits
    if _hist_limits is None:
        out = np.zeros(WN_HIST_BUCKETS, np.float64)
        n = load_library().wn_stats_hist_limits(out.ctypes.data_as(ctypes.c_void_p), WN_HIST_BUCKETS)
        if n != WN_HIST_BUCKETS:
            raise WnError(n, (load_library().wn_stats_last_error(None) or b'').decode())
        out.setflags(write=False)
        _hist_limits = out
    return _hist_limits


def stats_config(max_rows=0, max_time=0, max_tensors=0):
    cfg = WnStatsConfig()
    cfg.abi_version = WN_ABI_VERSION
    cfg.max_rows, cfg.max_time, cfg.max_tensors = int(max_rows), int(max_time), int(max_tensors)
    return cfg


def _hist_dict(bucket, summary):
    res = {'bucket': bucket}
    for k, v in zip(HIST_SUMMARY, summary):
        res[k] = float(v) if k in ('min', 'max', 'sum', 'sum_squares') else int(v)
    return res


def _hist_geometry(shape, channel, T=None):
    """(B, T, pitch in floats, offset in floats) of x [B, P] or of channel `channel` of x [B, O, P]; T: the rows' length (None: P; else 1 <= T <= P)"""
    P = int(shape[-1])
    T = P if T is None else int(T)
    if T > P:
        raise ValueError('T (%d) exceeds the last dimension (%d)' % (T, P))
    if channel is None:
        if len(shape) != 2:
            raise ValueError('x must be [B, T] (or [B, O, T] with channel=) (got %r)' % (tuple(shape),))
        return int(shape[0]), T, P, 0
    if len(shape) != 3 or not 0 <= int(channel) < int(shape[1]):
        raise ValueError('x must be [B, O, T] with 0 <= channel < O (got %r, channel %r)' % (tuple(shape), channel))
    return int(shape[0]), T, int(shape[1]) * P, int(channel) * P


def _tensor_table(tensors):
    """layout (name -> (shape, offset), Engine.layout) or [(offset, count)] -> names, int64 offsets, int64 counts"""
    if hasattr(tensors, 'items'):
        names = list(tensors)
        pairs = [(int(off), int(np.prod(shape))) for shape, off in tensors.values()]
    else:
        pairs = [(int(o), int(c)) for o, c in tensors]
        names = ['tensor_%d' % i for i in range(len(pairs))]
    return names, np.array([p[0] for p in pairs], np.int64), np.array([p[1] for p in pairs], np.int64)


class TrainStats:
    """One wn_stats: the histogram of a ragged batch and the per-tensor statistics of a flat buffer on the current device (csrc/wn_stats.hip), with
    pre-allocated outputs.  tensors: Engine.layout (name -> (shape, offset)) or [(offset, count)], set once.  max_rows = 0 gives a validation-only
    handle (no device; every run is refused); the *_host methods and encode / decode need no handle's device at all."""

    def __init__(self, max_rows, max_time, tensors=None):
        self.lib = load_library()
        self.names, self._off, self._cnt = _tensor_table(tensors) if tensors is not None else ([], np.zeros(0, np.int64), np.zeros(0, np.int64))
        self.cfg = stats_config(max_rows, max_time, len(self.names))
        h = ctypes.c_void_p()
        rc = self.lib.wn_stats_create(ctypes.byref(self.cfg), ctypes.byref(h))
        if rc != 0:
            raise WnError(rc, (self.lib.wn_stats_last_error(None) or b'').decode())
        self.h = h
        self.max_rows, self.max_time = int(max_rows), int(max_time)
        self._bucket = self._summary = self._tout = None
        if self.names:
            self._ok(self.lib.wn_stats_set_tensors(self.h, self._off.ctypes.data_as(ctypes.c_void_p), self._cnt.ctypes.data_as(ctypes.c_void_p), len(self.names)))
        if self.max_rows > 0:
            import torch
            self._bucket = torch.zeros(WN_HIST_BUCKETS, dtype=torch.int64, device='cuda')
            self._summary = torch.zeros(8, dtype=torch.float64, device='cuda')
            self._tout = torch.zeros(max(len(self.names), 1), 4, dtype=torch.float64, device='cuda')

    def _ok(self, rc):
        if rc != 0:
            raise WnError(rc, (self.lib.wn_stats_last_error(self.h) or b'').decode())

    def histogram(self, x, lengths=None, channel=None, T=None):
        """x float32 on the device, [B, T] or -- with channel -- [B, O, T] of which channel `channel` is taken; lengths: int32 [B] on the device (elements
        at t >= lengths[b] are not read) or None; T: the rows' length when the last dimension is a longer pitch.  Returns a dict on the host: 'bucket' int64 [WN_HIST_BUCKETS] and the HIST_SUMMARY fields.  Waits for
        the device (one copy of 12 KB)."""
        import torch
        _check(x, torch.float32, 'x')
        B, T, pitch, off = _hist_geometry(x.shape, channel, T)
        if lengths is not None:
            _check(lengths, torch.int32, 'lengths')
            if int(lengths.numel()) != B:
                raise ValueError('lengths must have one entry per row')
        self._ok(self.lib.wn_stats_histogram(self.h, ctypes.c_void_p(x.data_ptr() + 4 * off), pitch, _ptr(lengths), B, T, _ptr(self._bucket), _ptr(self._summary), _stream()))
        return _hist_dict(self._bucket.cpu().numpy(), self._summary.cpu().numpy())

    def tensor_stats(self, flat):
        """flat: float32 on the device, covering every tensor of the table.  Returns float64 [nt, 4] on the host (TENSOR_STATS).  Waits for the device."""
        import torch
        _check(flat, torch.float32, 'flat')
        if not self.names:
            raise ValueError('TrainStats.tensor_stats: the handle was created without a tensor table')
        if int((self._off + self._cnt).max()) > int(flat.numel()):
            raise ValueError('flat has %d elements, the tensor table reaches %d' % (int(flat.numel()), int((self._off + self._cnt).max())))
        self._ok(self.lib.wn_stats_tensors(self.h, _ptr(flat), _ptr(self._tout), _stream()))
        return self._tout[:len(self.names)].cpu().numpy()

    @staticmethod
    def histogram_host(x, lengths=None, channel=None, T=None):
        """wn_test_stats_hist_host: histogram() of numpy float32 data on the host (no GPU), in the device's order: the same bits."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        B, T, pitch, off = _hist_geometry(x.shape, channel, T)
        ln = None
        if lengths is not None:
            ln = np.ascontiguousarray(lengths, dtype=np.int32)
            if ln.size != B:
                raise ValueError('lengths must have one entry per row')
        bucket, summary = np.full(WN_HIST_BUCKETS, -1, np.int64), np.full(8, np.nan, np.float64)
        vp = ctypes.c_void_p
        rc = load_library().wn_test_stats_hist_host(vp(x.ctypes.data + 4 * off), pitch, None if ln is None else ln.ctypes.data_as(vp), B, T,
                                                    bucket.ctypes.data_as(vp), summary.ctypes.data_as(vp))
        if rc != 0:
            raise WnError(rc, (load_library().wn_stats_last_error(None) or b'').decode())
        return _hist_dict(bucket, summary)

    @staticmethod
    def tensor_stats_host(flat, tensors):
        """wn_test_stats_tensors_host: tensor_stats() of a numpy float32 buffer on the host (no GPU), in the device's order."""
        flat = np.ascontiguousarray(flat, dtype=np.float32)
        _, off, cnt = _tensor_table(tensors)
        if off.size and int((off + cnt).max()) > flat.size:
            raise ValueError('flat has %d elements, the tensor table reaches %d' % (flat.size, int((off + cnt).max())))
        out = np.full((max(off.size, 1), 4), np.nan, np.float64)
        vp = ctypes.c_void_p
        rc = load_library().wn_test_stats_tensors_host(flat.ctypes.data_as(vp), off.ctypes.data_as(vp), cnt.ctypes.data_as(vp), int(off.size), out.ctypes.data_as(vp))
        if rc != 0:
            raise WnError(rc, (load_library().wn_stats_last_error(None) or b'').decode())
        return out[:off.size]

    @staticmethod
    def encode(hist):
        """A histogram dict as TensorFlow encodes a HistogramProto: min, max, num, sum, sum_squares, and bucket_limit / bucket with every run of empty
        buckets collapsed into ONE zero entry that carries the run's last limit, so only limits of non-empty buckets (and of the ends of empty runs)
        appear.  Plain floats and ints: a JSON row."""
        limits, counts = hist_limits(), hist['bucket']
        lim, cnt, i, n = [], [], 0, len(counts)
        while i < n:
            end, c = float(limits[i]), int(counts[i])
            i += 1
            if c <= 0:
                while i < n and counts[i] <= 0:
                    end, c = float(limits[i]), int(counts[i])
                    i += 1
            lim.append(end); cnt.append(c)
        res = {k: (float(hist[k]) if k in ('min', 'max', 'sum', 'sum_squares') else int(hist[k])) for k in HIST_SUMMARY}
        res['bucket_limit'], res['bucket'] = lim, cnt
        return res

    @staticmethod
    def decode(enc):
        """The int64 [WN_HIST_BUCKETS] counts of an encode()d histogram."""
        limits = hist_limits()
        out = np.zeros(WN_HIST_BUCKETS, np.int64)
        for end, c in zip(enc['bucket_limit'], enc['bucket']):
            if c:
                i = int(np.searchsorted(limits, end, side='left'))
                if i >= WN_HIST_BUCKETS or limits[i] != end:
                    raise ValueError('bucket_limit %r is no limit of the table' % (end,))
                out[i] = int(c)
        return out

    def close(self):
        if getattr(self, 'h', None):
            self.lib.wn_stats_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
