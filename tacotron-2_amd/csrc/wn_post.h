// Output stage arithmetic shared by the device kernels of wn_post.hip, the unfold kernel of wn_fold.hip (the decode), the host hook wn_test_post_host
// and the stand-alone host program tests/host/post_main.cpp: the decode of a model-domain sample, one step of the de-emphasis chain, the conversion to
// 16-bit PCM and the validation of a configuration and of a call.  Everything here is written once and runs on either side.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/wavenet_mi355.h"

// The decode table lives in device memory (wn_mulaw_tables.h: __device__ static const).  The host side of a translation unit that decodes on the host
// (wn_post.hip's hook, post_main.cpp) sees the same initialiser as an ordinary constant array: define WN_POST_HOST_TABLES before the first inclusion.
#if defined(WN_POST_HOST_TABLES) && !defined(__HIP_DEVICE_COMPILE__)
#pragma push_macro("__device__")
#undef __device__
#define __device__
#include "wn_mulaw_tables.h"
#pragma pop_macro("__device__")
#else
#include "wn_mulaw_tables.h"
#endif

// decode of a model-domain sample given as its 32 bits: the arithmetic of wn_inv_mulaw_kernel / wn_inv_mulaw_quantize_kernel (wn_loss.hip), identity for 'raw'
template <int TYPE> __host__ __device__ __forceinline__ float wn_decode_sample(int32_t bits) {
    if (TYPE == WN_INPUT_MULAW_QUANTIZE) return WN_MULAW_DECODE[bits < 0 ? 0 : bits > 255 ? 255 : bits];
    const float v = __builtin_bit_cast(float, bits);
    if (TYPE == WN_INPUT_RAW) return v;
    const float s = (v > 0.0f) ? 1.0f : (v < 0.0f ? -1.0f : 0.0f);
    return (float)((double)s * (1.0 / 255.0) * (pow(256.0, fabs((double)v)) - 1.0));
}
__host__ __device__ __forceinline__ float wn_post_decode(int type, int32_t bits) {
    return type == WN_INPUT_MULAW_QUANTIZE ? wn_decode_sample<WN_INPUT_MULAW_QUANTIZE>(bits) : type == WN_INPUT_MULAW ? wn_decode_sample<WN_INPUT_MULAW>(bits) : wn_decode_sample<WN_INPUT_RAW>(bits);
}

// y[t] = fl32(fl32(k y[t - 1]) + x[t]): one multiply and one add, each rounded, never one fma
// (not __fmul_rn / __fadd_rn: in this toolchain's headers they are a plain * and + that carry the default -ffp-contract=fast with them when they are
// inlined, and the pair came out as one v_fma_f32.  Operators under the pragma keep the two roundings, on both sides -- as fold_xfade does)
__host__ __device__ __forceinline__ float wn_post_step(float k, float y_prev, float x) {
#pragma clang fp contract(off)
    const float m = k * y_prev;
    return m + x;
}

// v = fl32(y s); the sample is v clamped to [-32767, 32767] and truncated toward zero (numpy's astype(int16) on a value in range); clipped: |v| > 32767
__host__ __device__ __forceinline__ int16_t wn_post_pcm(float y, float s, int32_t* clipped) {
#if defined(__HIP_DEVICE_COMPILE__)
    const float v = __fmul_rn(y, s);
#else
    const float v = y * s;
#endif
    *clipped += (fabsf(v) > 32767.0f) ? 1 : 0;
    const float c = v > 32767.0f ? 32767.0f : v < -32767.0f ? -32767.0f : v;      // (a NaN passes both comparisons and converts below)
    return (int16_t)(int32_t)(c == c ? c : 0.0f);
}
// the scale of wn_post_push (gain in double on the host) and of wn_post_finish (save_wavenet_wav: 32767 / max(0.01, peak), in double)
__host__ __device__ __forceinline__ float wn_post_gain_scale(float gain) { return (float)((double)gain * 32767.0); }
__host__ __device__ __forceinline__ float wn_post_peak_scale(float peak) { const double p = (double)peak; return (float)(32767.0 / (p > 0.01 ? p : 0.01)); }

// ---- host: the whole stage over one row in sample order (the hook and post_main.cpp), and the validation every entry point runs before any device call
static inline void wn_post_host_row(int type, float k, const void* in, int64_t n, float carry_in, float pcm_scale, float* out_f32, int16_t* out_pcm, float* carry_out,
                                    float* peak, int32_t* clipped) {
    float y = carry_in, pk = 0.0f;
    int32_t nclip = 0;
    const int32_t* bits = (const int32_t*)in;
    for (int64_t t = 0; t < n; ++t) {
        const float x = wn_post_decode(type, bits[t]);
        y = k == 0.0f ? x : wn_post_step(k, y, x);
        const float a = fabsf(y);
        if (a > pk) pk = a;
        if (out_f32) out_f32[t] = y;
        if (out_pcm) out_pcm[t] = wn_post_pcm(y, pcm_scale, &nclip);
    }
    if (carry_out) *carry_out = y;
    if (peak) *peak = pk;
    if (clipped) *clipped = nclip;
}

#define WN_POST_FAIL(code, ...) do { if (msg && cap > 0) snprintf(msg, (size_t)cap, __VA_ARGS__); return (code); } while (0)

static inline int wn_post_check_config(const wn_post_config* cfg, char* msg, int cap) {
    if (!cfg) WN_POST_FAIL(WN_E_ARG, "null configuration");
    if (cfg->abi_version != WN_ABI_VERSION) WN_POST_FAIL(WN_E_ARG, "abi_version %d != %d", cfg->abi_version, WN_ABI_VERSION);
    if (cfg->max_rows < 1) WN_POST_FAIL(WN_E_ARG, "max_rows (%d) must be >= 1", cfg->max_rows);
    if (cfg->in_type < 0 || cfg->in_type > 2) WN_POST_FAIL(WN_E_ARG, "in_type (%d) must be 0 (float waveform), 1 (float mu-law) or 2 (int32 class ids)", cfg->in_type);
    if (!(cfg->deemphasis >= 0.0f && cfg->deemphasis < 1.0f)) WN_POST_FAIL(WN_E_ARG, "deemphasis (%g) must be in [0, 1)", (double)cfg->deemphasis);
    if (!(cfg->gain > 0.0f) || isinf(cfg->gain)) WN_POST_FAIL(WN_E_ARG, "gain (%g) must be finite and > 0", (double)cfg->gain);
    return WN_OK;
}
// one call of wn_post_push (finish = 0: either output) or wn_post_finish (finish = 1: out_f32 required)
static inline int wn_post_check_call(const char* who, int finish, int32_t max_rows, const void* in, int64_t in_pitch, const int32_t* n, int32_t B, const float* out_f32,
                                     const int16_t* out_pcm, int64_t out_pitch, char* msg, int cap) {
    if (!in || !n) WN_POST_FAIL(WN_E_ARG, "%s: null argument", who);
    if (finish && !out_f32) WN_POST_FAIL(WN_E_ARG, "%s: out_f32 is required", who);
    if (!finish && !out_f32 && !out_pcm) WN_POST_FAIL(WN_E_ARG, "%s: both outputs are null", who);
    if (B < 1) WN_POST_FAIL(WN_E_ARG, "%s: B (%d) must be >= 1", who, B);
    if (B > max_rows) WN_POST_FAIL(WN_E_SHAPE, "%s: B (%d) > max_rows = %d", who, B, max_rows);
    int32_t n_max = 0;
    for (int b = 0; b < B; ++b) {
        if (n[b] < 0) WN_POST_FAIL(WN_E_ARG, "%s: n[%d] = %d is negative", who, b, n[b]);
        if (n[b] > n_max) n_max = n[b];
    }
    if (in_pitch < n_max) WN_POST_FAIL(WN_E_SHAPE, "%s: in_pitch (%lld) < the longest row (%d)", who, (long long)in_pitch, n_max);
    if (out_pitch < n_max) WN_POST_FAIL(WN_E_SHAPE, "%s: out_pitch (%lld) < the longest row (%d)", who, (long long)out_pitch, n_max);
    return WN_OK;
}
