// Spectral denoiser arithmetic shared by the device kernels of wn_denoise.hip, the host hook wn_test_denoise_host and the stand-alone host program
// tests/host/denoise_main.cpp: the geometry of a tile, the two basis tables, the shrink of one bin, the validation of a configuration and of a call, and
// the whole operation on host arrays in plain float32.
//
// Geometry: n_fft, hop, periodic Hann w[j] = 0.5 - 0.5 cos(2 pi j / n_fft).  F = 1 + n / hop frames, frame f = the n_fft samples centred on f hop, zeros
// outside [0, n) (the frames of wn_mel).  With H = n_fft / 2:
//   analysis   X[f][k] = sum_j w[j] x[f hop - H + j] e^{-2 pi i j k / n_fft}, k = 0 ... H
//   shrink     m = |X|, t = strength profile[k]; Y = X (m - t) / m where m > t, else 0
//   synthesis  y_f[j] = w[j] irfft(Y[f])[j];  out[i] = (sum_f y_f[i - f hop + H]) / (sum_f w[i - f hop + H]^2), covering frames ascending
//   profile    mean of |X[f][k]| over the frames whose window lies inside [0, n): f hop >= H and f hop + H <= n; rows ascending, frames ascending
// hop <= n_fft / 4 puts every sample within n_fft / 4 of a frame centre, where w >= 0.5: the window-square sum is >= 0.25 for every n >= 1.
//
// The real spectrum is kept PACKED in n_fft floats per frame: bins 0 and H have no imaginary part (their sine columns are exactly zero), so the real part
// of bin H rides in the imaginary slot of bin 0.  Packed column c = 2 k + {0: re, 1: im} for k = 0 ... H - 1, with c = 1 holding Re X[H]: the forward
// product has H (not H + 1) complex columns, the inverse product has K = n_fft rows.  Both tables are built in double with the angle reduced as the
// integer (j k) mod n_fft and rounded to float32 once.
//
// What the tiling holds (WN_E_UNSUPPORTED otherwise): n_fft a multiple of 32 (whole 32-column groups of the inverse product) and n_fft <= 4096 (the
// signal span of a 32-frame tile, 31 hop + n_fft floats with hop <= n_fft / 4, and the fit patch fit the 160 KiB of LDS).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <vector>

#include "../../include/wavenet_mi355.h"

#define DN_TILE 32             // frames per workgroup
#define DN_THREADS 256
#define DN_GROUP 64            // rows per launch: their lengths travel as kernel arguments
#define DN_MAX_FFT 4096
#define DN_PATCH 34            // pitch of a wave's [32 frames][32 bins + Nyquist] magnitude patch (fit)

static inline int dn_bins(int n_fft) { return 1 + n_fft / 2; }
static inline int dn_groups(int n_fft) { return (n_fft / 2 + 31) / 32; }                  // 32-bin groups of the forward product (bins 0 ... H - 1)
static inline int64_t dn_sig_floats(int64_t n_fft, int64_t hop) { return (DN_TILE - 1) * hop + n_fft; }
static inline int64_t dn_lds_floats(int64_t n_fft, int64_t hop) { return dn_sig_floats(n_fft, hop) + 4 * DN_TILE * DN_PATCH; }
static inline int64_t dn_frames_padded(int64_t max_samples, int64_t hop) { return (1 + max_samples / hop + DN_TILE - 1) / DN_TILE * DN_TILE; }
// where the shrink stores packed column c = 2 k + ri of a frame's row: blocks of 8 columns as [re of bins 4 q ... 4 q + 3 | im of the same], so that the
// lane that feeds (re, im) of four consecutive bins to the inverse product reads them as one 16-byte word
__host__ __device__ __forceinline__ int dn_spec_slot(int k, int ri) { return (k >> 2) * 8 + ri * 4 + (k & 3); }

// one bin: two roundings for the power, sqrt, subtract, divide, two products -- the same on both sides
__host__ __device__ __forceinline__ void dn_shrink(float re, float im, float t, float* yr, float* yi) {
#pragma clang fp contract(off)
    const float m = sqrtf(re * re + im * im);
    const float s = m > t ? (m - t) / m : 0.0f;
    *yr = re * s; *yi = im * s;
}
__host__ __device__ __forceinline__ float dn_mag(float re, float im) {
#pragma clang fp contract(off)
    return sqrtf(re * re + im * im);
}

// ---- host: the tables
struct DnTables {
    int n_fft = 0, G = 0, ldb = 0;
    std::vector<float> fb;       // [n_fft taps][G][re 32 | im 32]: w[j] cos, -w[j] sin of bin 32 g + q; the im column of bin 0 holds bin H's w[j] cos(pi j)
    std::vector<float> ib;       // [n_fft packed columns][n_fft samples]: synthesis window, Hermitian weight (1 for bins 0 and H, 2 elsewhere) and 1 / n_fft folded in
    std::vector<float> wsq;      // w[j]^2
};
static inline void dn_build_tables(int n_fft, DnTables* t) {
    const int H = n_fft / 2;
    t->n_fft = n_fft; t->G = dn_groups(n_fft); t->ldb = t->G * 64;
    t->fb.assign((size_t)n_fft * t->ldb, 0.0f);
    t->ib.assign((size_t)n_fft * n_fft, 0.0f);
    t->wsq.assign((size_t)n_fft, 0.0f);
    std::vector<double> ct(n_fft), st(n_fft), w(n_fft);
    const double two_pi = 6.283185307179586476925286766559;
    for (int i = 0; i < n_fft; ++i) { ct[i] = cos(two_pi * i / n_fft); st[i] = sin(two_pi * i / n_fft); w[i] = 0.5 - 0.5 * ct[i]; }
    for (int j = 0; j < n_fft; ++j) {
        t->wsq[j] = (float)(w[j] * w[j]);
        for (int k = 0; k < H; ++k) {
            const int idx = (int)(((int64_t)j * k) % n_fft);
            float* p = &t->fb[(size_t)j * t->ldb + (k / 32) * 64 + (k % 32)];
            const double sign = (j & 1) ? -1.0 : 1.0;      // cos(pi j)
            p[0] = (float)(w[j] * ct[idx]);
            p[32] = k == 0 ? (float)(w[j] * sign) : (float)(-w[j] * st[idx]);
            const double h = k == 0 ? 1.0 : 2.0;
            t->ib[(size_t)(2 * k) * n_fft + j] = (float)(w[j] * h * ct[idx] / n_fft);
            t->ib[(size_t)(2 * k + 1) * n_fft + j] = k == 0 ? (float)(w[j] * sign / n_fft) : (float)(-w[j] * h * st[idx] / n_fft);
        }
    }
}

// ---- validation: what every entry point runs before any device call
#define WN_DN_FAIL(code, ...) do { if (msg && cap > 0) snprintf(msg, (size_t)cap, __VA_ARGS__); return (code); } while (0)

static inline int wn_denoise_check_config(const wn_denoise_config* cfg, char* msg, int cap) {
    if (!cfg) WN_DN_FAIL(WN_E_ARG, "null configuration");
    if (cfg->abi_version != WN_ABI_VERSION) WN_DN_FAIL(WN_E_ARG, "abi_version %d != %d", cfg->abi_version, WN_ABI_VERSION);
    if (cfg->max_batch < 0 || cfg->max_samples < 0 || cfg->max_samples > 0x7fffffffLL) WN_DN_FAIL(WN_E_ARG, "max_batch / max_samples must be in [0, 2^31)");
    if (cfg->n_fft < 8 || cfg->n_fft % 2) WN_DN_FAIL(WN_E_SHAPE, "n_fft (%d) must be even and >= 8", cfg->n_fft);
    if (cfg->hop < 1 || cfg->hop > cfg->n_fft / 4) WN_DN_FAIL(WN_E_SHAPE, "hop (%d) must be in [1, n_fft / 4 = %d]", cfg->hop, cfg->n_fft / 4);
    if (cfg->n_fft % 32 || cfg->n_fft > DN_MAX_FFT)
        WN_DN_FAIL(WN_E_UNSUPPORTED, "n_fft (%d) must be a multiple of 32 and <= %d: the inverse product runs in whole 32-column groups and a 32-frame tile's span must fit the LDS",
                   cfg->n_fft, DN_MAX_FFT);
    return WN_OK;
}
// argument errors of a batch (fit and run alike); out may be the input
static inline int wn_denoise_check_args(const char* who, const float* wav, int64_t pitch, const int32_t* lengths, int32_t B, char* msg, int cap) {
    if (!wav || !lengths) WN_DN_FAIL(WN_E_ARG, "%s: null argument", who);
    if (B < 1) WN_DN_FAIL(WN_E_ARG, "%s: B (%d) must be >= 1", who, B);
    if (pitch < 0) WN_DN_FAIL(WN_E_ARG, "%s: pitch (%lld) is negative", who, (long long)pitch);
    for (int b = 0; b < B; ++b)
        if (lengths[b] < 0) WN_DN_FAIL(WN_E_ARG, "%s: lengths[%d] = %d is negative", who, b, lengths[b]);
    return WN_OK;
}
// shapes of a batch; max_batch < 0: no limit on B and max_samples (the host hook)
static inline int wn_denoise_check_shape(const char* who, int32_t max_batch, int64_t max_samples, int64_t pitch, const int32_t* lengths, int32_t B, char* msg, int cap) {
    if (max_batch >= 0 && B > max_batch) WN_DN_FAIL(WN_E_SHAPE, "%s: B (%d) > max_batch = %d", who, B, max_batch);
    for (int b = 0; b < B; ++b) {
        if (lengths[b] > pitch) WN_DN_FAIL(WN_E_SHAPE, "%s: lengths[%d] = %d > pitch = %lld", who, b, lengths[b], (long long)pitch);
        if (max_batch >= 0 && lengths[b] > max_samples) WN_DN_FAIL(WN_E_SHAPE, "%s: lengths[%d] = %d exceeds max_samples = %lld", who, b, lengths[b], (long long)max_samples);
    }
    return WN_OK;
}
static inline int wn_denoise_check_strength(const char* who, float strength, char* msg, int cap) {
    if (!(strength >= 0.0f) || isinf(strength)) WN_DN_FAIL(WN_E_ARG, "%s: strength (%g) must be finite and >= 0", who, (double)strength);
    return WN_OK;
}
static inline int wn_denoise_check_profile(const char* who, const float* profile, int nb, char* msg, int cap) {
    if (!profile) WN_DN_FAIL(WN_E_ARG, "%s: null argument", who);
    for (int k = 0; k < nb; ++k)
        if (!(profile[k] >= 0.0f) || isinf(profile[k])) WN_DN_FAIL(WN_E_ARG, "%s: profile[%d] = %g must be finite and >= 0", who, k, (double)profile[k]);
    return WN_OK;
}
// frames of a row of n samples whose window lies inside [0, n)
static inline int64_t wn_denoise_fit_frames(int64_t n, int64_t n_fft, int64_t hop) {
    const int64_t H = n_fft / 2;
    if (n < n_fft) return 0;
    return (n - H) / hop - (H + hop - 1) / hop + 1;      // f from ceil(H / hop) to floor((n - H) / hop)
}

// ---- host: the operation in plain float32 on the tables above, in the device's order: fused multiply-adds ascending in the device's interleaved chains
// (the forward sum in two, tap pair (j >> 1) & 1; the inverse sum in four, packed column pair (c >> 1) & 3), joined as the kernels join them
// X of one frame, packed: spec[2 k], spec[2 k + 1] = re, im of bin k (spec[1] = Re X[H]); spec holds 2 n_fft floats (the second half is scratch).
// Reads wav[s] for 0 <= s < n only.  dn_host_analyse_at: wav holds the samples from `base` on (sample s at wav[s - base]; the streaming form keeps only a
// row's tail) and every sample the frame needs below n lies at or above base.
static inline void dn_host_analyse_at(const DnTables& t, int hop, const float* wav, int64_t base, int64_t n, int64_t f, float* spec) {
#pragma clang fp contract(off)
    const int N = t.n_fft, H = N / 2;
    const int64_t s0 = f * hop - H;
    for (int c = 0; c < 2 * N; ++c) spec[c] = 0.0f;
    for (int j = 0; j < N; ++j) {
        const int64_t s = s0 + j;
        if (s < 0 || s >= n) continue;      // a zero sample adds exactly nothing
        const float x = wav[s - base];
        const float* row = &t.fb[(size_t)j * t.ldb];
        float* acc = spec + ((j >> 1) & 1) * N;
        for (int k = 0; k < H; ++k) {
            const float* p = row + (k / 32) * 64 + (k % 32);
            acc[2 * k] = __builtin_fmaf(x, p[0], acc[2 * k]);
            acc[2 * k + 1] = __builtin_fmaf(x, p[32], acc[2 * k + 1]);
        }
    }
    for (int c = 0; c < N; ++c) spec[c] = spec[c] + spec[N + c];
}
static inline void dn_host_analyse(const DnTables& t, int hop, const float* wav, int64_t n, int64_t f, float* spec) { dn_host_analyse_at(t, hop, wav, 0, n, f, spec); }
// one analysed frame (spec, packed; shrunk in place) -> its windowed frame y [n_fft]; ch: 4 n_fft floats of scratch (the four chains of the inverse sum)
static inline void dn_host_synth_frame(const DnTables& t, const float* profile, float strength, float* spec, float* ch, float* y) {
#pragma clang fp contract(off)
    const int N = t.n_fft, H = N / 2;
    float d;
    dn_shrink(spec[0], 0.0f, strength * profile[0], &spec[0], &d);
    dn_shrink(spec[1], 0.0f, strength * profile[H], &spec[1], &d);
    for (int k = 1; k < H; ++k) dn_shrink(spec[2 * k], spec[2 * k + 1], strength * profile[k], &spec[2 * k], &spec[2 * k + 1]);
    for (size_t e = 0; e < (size_t)4 * N; ++e) ch[e] = 0.0f;
    for (int c = 0; c < N; ++c) {
        const float v = spec[c];
        const float* row = &t.ib[(size_t)c * N];
        float* acc = &ch[(size_t)((c >> 1) & 3) * N];
        for (int j = 0; j < N; ++j) acc[j] = __builtin_fmaf(v, row[j], acc[j]);
    }
    for (int j = 0; j < N; ++j) y[j] = (ch[j] + ch[N + j]) + (ch[2 * (size_t)N + j] + ch[3 * (size_t)N + j]);
}
// the mean magnitude of the wholly-inside frames of B rows -> profile [H + 1]; returns the number of frames (0: nothing written)
static inline int64_t wn_denoise_host_fit(const DnTables& t, int hop, const float* wav, int64_t ld, const int32_t* lengths, int32_t B, float* profile) {
    const int N = t.n_fft, H = N / 2;
    std::vector<double> sum((size_t)H + 1, 0.0);
    std::vector<float> spec((size_t)2 * N), part((size_t)H + 1);
    int64_t count = 0;
    for (int64_t b = 0; b < B; ++b) {
        const int64_t n = lengths[b], F = 1 + n / hop;
        for (int64_t f0 = 0; f0 < F; f0 += DN_TILE) {      // the device's order: float32 partial sums per tile of 32 frames, joined in double
            for (int k = 0; k <= H; ++k) part[k] = 0.0f;
            for (int64_t f = f0; f < F && f < f0 + DN_TILE; ++f) {
                if (f * hop < H || f * hop + H > n) continue;
                dn_host_analyse(t, hop, wav + b * ld, n, f, spec.data());
                part[0] = part[0] + fabsf(spec[0]);
                part[H] = part[H] + fabsf(spec[1]);
                for (int k = 1; k < H; ++k) part[k] = part[k] + dn_mag(spec[2 * k], spec[2 * k + 1]);
                ++count;
            }
            for (int k = 0; k <= H; ++k) sum[k] += (double)part[k];
        }
    }
    if (count == 0) return 0;
    for (int k = 0; k <= H; ++k) profile[k] = (float)(sum[k] / (double)count);
    return count;
}
// rows of in -> rows of out (in == out allowed); writes out[b * out_pitch + i] for i < lengths[b] only
static inline void wn_denoise_host_run(const DnTables& t, int hop, const float* profile, const float* in, int64_t in_pitch, const int32_t* lengths, int32_t B, float strength,
                                       float* out, int64_t out_pitch) {
#pragma clang fp contract(off)
    const int N = t.n_fft, H = N / 2;
    std::vector<float> spec((size_t)2 * N), fr, ch((size_t)4 * N);
    for (int64_t b = 0; b < B; ++b) {
        const int64_t n = lengths[b], F = 1 + n / hop;
        if (n == 0) continue;
        fr.assign((size_t)F * N, 0.0f);
        for (int64_t f = 0; f < F; ++f) {
            dn_host_analyse(t, hop, in + b * in_pitch, n, f, spec.data());
            dn_host_synth_frame(t, profile, strength, spec.data(), ch.data(), &fr[(size_t)f * N]);
        }
        for (int64_t i = 0; i < n; ++i) {
            const int64_t f_lo = i >= H ? (i - H) / hop + 1 : 0, f_hi = (i + H) / hop < F - 1 ? (i + H) / hop : F - 1;
            float num = 0.0f, den = 0.0f;
            for (int64_t f = f_lo; f <= f_hi; ++f) { const int64_t j = i - f * hop + H; num = num + fr[(size_t)f * N + j]; den = den + t.wsq[j]; }
            out[b * out_pitch + i] = num / den;
        }
    }
}

// library-internal (not part of the C ABI): where a handle's profile lives -- the device array of a handle with rows, the host copy of a geometry-only
// one; WN_E_STATE before any profile.  wn_denoise_stream_take_profile reads it.
extern "C" int wn_denoise_profile_source(const wn_denoise* h, int32_t* n_fft, const float** device_profile, const float** host_profile);
