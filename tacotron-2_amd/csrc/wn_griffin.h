// Griffin-Lim arithmetic shared by the device kernels of wn_griffin.hip, the host hook wn_test_griffin_host and the stand-alone host program
// tests/host/griffin_main.cpp: the geometry, the two basis tables, the mel -> magnitude map, the projection of one bin, the validation of a configuration
// and of a call, and the whole operation on host arrays in plain float32.
//
// Geometry: n_fft = N, win_size = W <= N, hop; H = N / 2, off = (N - W) / 2, Hl = H - off.  Window: periodic Hann of W, w[t] = 0.5 - 0.5 cos(2 pi t / W),
// centred in N (tap t of the window is position off + t of the frame; the rest of the frame is zero).  A row of F frames is a signal of n = hop (F - 1)
// samples; frame f is centred on f hop, zeros outside [0, n) (the frames of wn_mel: 1 + n / hop = F of them).
//   analysis    X[f][k] = sum_t w[t] y[f hop - Hl + t] e^{-2 pi i (off + t) k / N},  k = 0 ... H       (only the W taps the window leaves non-zero)
//   projection  Y = S X / |X|; an exactly zero X takes the phase (1, 0); bins 0 and H are real: Y = +-S
//   synthesis   y_f[t] = w[t] irfft(Y[f])[off + t], t = 0 ... W - 1                                      (only the W samples the window leaves non-zero)
//               y[i] = (sum_f y_f[i + Hl - f hop]) / (sum_f w[i + Hl - f hop]^2), covering frames ascending -- librosa's istft after its trim of N / 2
// hop <= W / 4 puts every sample of [0, n) within W / 8 of a frame centre, where w > 0.85: the window-square sum is positive for every F >= 2.
//
// The spectrum is kept PACKED in N floats per frame as the denoiser's (wn_denoise.h): the real part of bin H rides in the imaginary slot of bin 0, packed
// column c = 2 k + {0: re, 1: im}, stored in blocks of 8 as [re of bins 4 q ... 4 q + 3 | im of the same] (gl_spec_slot).  The forward table has Wp = W
// rounded up to 8 rows (taps), the inverse table N rows (packed columns) of ldi = W rounded up to 32 samples; both are built in double with the angle
// reduced as an integer mod N and rounded to float32 once.  The product loops are COPIES of wn_denoise_dev.h's (same chains, same joins) with the tap
// count and the row pitch of the inverse table as parameters; the denoiser's own translation units do not include this file.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <vector>

#include "../../include/wavenet_mi355.h"

#define GL_TILE 32             // frames per workgroup
#define GL_THREADS 256
#define GL_GROUP 64            // rows per launch: their frame counts travel as kernel arguments
#define GL_MAX_FFT 4096
#define GL_MAX_MELS 512

struct GlGeom { int N = 0, W = 0, hop = 0, H = 0, NB = 0, off = 0, Hl = 0, Wp = 0, G = 0, ldb = 0, ldi = 0; };
static inline GlGeom gl_geom(int n_fft, int win_size, int hop) {
    GlGeom g;
    g.N = n_fft; g.W = win_size; g.hop = hop; g.H = n_fft / 2; g.NB = g.H + 1; g.off = (n_fft - win_size) / 2; g.Hl = g.H - g.off;
    g.Wp = (win_size + 7) / 8 * 8; g.G = (g.H + 31) / 32; g.ldb = g.G * 64; g.ldi = (win_size + 31) / 32 * 32;
    return g;
}
static inline int64_t gl_sig_floats(const GlGeom& g) { return (int64_t)(GL_TILE - 1) * g.hop + g.Wp; }
static inline int64_t gl_frames_padded(int64_t frames) { return (frames + GL_TILE - 1) / GL_TILE * GL_TILE; }
__host__ __device__ __forceinline__ int gl_spec_slot(int k, int ri) { return (k >> 2) * 8 + ri * 4 + (k & 3); }
// multiply-adds of one iteration of one frame (both products, the packed formulation): what tools/griffin_timing.py counts
static inline int64_t gl_frame_macs(const GlGeom& g) { return (int64_t)g.Wp * g.G * 64 + (int64_t)g.N * g.ldi; }

// ---- the element-wise maps, the same text on both sides
// S (re, im) / hypot(re, im) with the larger component scaled to 1 first: no square underflows unless the other is 1
__host__ __device__ __forceinline__ void gl_project(float re, float im, float S, float* yr, float* yi) {
#pragma clang fp contract(off)
    const float m = fmaxf(fabsf(re), fabsf(im));
    if (!(m > 0.0f)) { *yr = S; *yi = 0.0f; return; }
    const float r = re / m, i = im / m;
    const float h = sqrtf(r * r + i * i);
    *yr = S * (r / h); *yi = S * (i / h);
}
__host__ __device__ __forceinline__ float gl_project_real(float re, float S) { return re < 0.0f ? -S : S; }
// the start: S e^{2 pi i u}
__host__ __device__ __forceinline__ void gl_start(float S, float u, float* yr, float* yi) {
#pragma clang fp contract(off)
    const float a = 6.28318530717958647692f * u;
    *yr = S * cosf(a); *yi = S * sinf(a);
}

// what the magnitude launch needs of a configuration (reference audio.py:97-104, 231-235, 252-253, 272-284)
struct GlMelMap { float lo, ref_db, maxabs, inv_mp, power; int32_t norm, clip, symmetric, num_mels; };
static inline GlMelMap gl_mel_map(const wn_griffin_config& c) {
    GlMelMap m;
    m.lo = c.min_level_db; m.ref_db = c.ref_level_db; m.maxabs = c.max_abs_value; m.inv_mp = 1.0f / c.magnitude_power; m.power = c.power;
    m.norm = c.signal_normalization != 0; m.clip = c.allow_clipping != 0; m.symmetric = c.symmetric_mels != 0; m.num_mels = c.num_mels;
    return m;
}
// one normalised mel value -> its linear amplitude: _denormalize, + ref_level_db, 10^(. / 20), ^(1 / magnitude_power)
__host__ __device__ __forceinline__ float gl_mel_amp(const GlMelMap& a, float D) {
#pragma clang fp contract(off)
    float S = D;
    if (a.norm) {
        if (a.clip) D = fminf(fmaxf(D, a.symmetric ? -a.maxabs : 0.0f), a.maxabs);
        S = a.symmetric ? ((D + a.maxabs) * -a.lo) / (2.0f * a.maxabs) + a.lo : (D * -a.lo) / a.maxabs + a.lo;
    }
    float v = powf(10.0f, (S + a.ref_db) * 0.05f);
    if (a.inv_mp != 1.0f) v = powf(v, a.inv_mp);
    return v;
}
// bin k of a frame from its num_mels amplitudes: pinvT [num_mels][NB], mels ascending in one chain of fused multiply-adds, max(1e-10, .), ^ power
__host__ __device__ __forceinline__ float gl_mel_bin(const GlMelMap& a, const float* amp, const float* pinvT, int NB, int k) {
    float s = 0.0f;
    for (int m = 0; m < a.num_mels; ++m) s = __builtin_fmaf(pinvT[(size_t)m * NB + k], amp[m], s);
    s = fmaxf(1e-10f, s);
    return a.power == 1.0f ? s : powf(s, a.power);
}

// ---- host: the tables
struct GlTables {
    GlGeom g;
    std::vector<float> fb;       // [Wp taps][G][re 32 | im 32]: w[t] cos, -w[t] sin of bin 32 q + c at position off + t; the im column of bin 0 holds bin H
    std::vector<float> ib;       // [N packed columns][ldi samples]: synthesis window, Hermitian weight (1 for bins 0 and H, 2 elsewhere) and 1 / N folded in
    std::vector<float> wsq;      // [ldi] w[t]^2, zero beyond W
};
static inline void gl_build_tables(int n_fft, int win_size, int hop, GlTables* t) {
    const GlGeom g = gl_geom(n_fft, win_size, hop);
    const int N = g.N, H = g.H;
    t->g = g;
    t->fb.assign((size_t)g.Wp * g.ldb, 0.0f);
    t->ib.assign((size_t)N * g.ldi, 0.0f);
    t->wsq.assign((size_t)g.ldi, 0.0f);
    std::vector<double> ct(N), st(N);
    const double two_pi = 6.283185307179586476925286766559;
    for (int i = 0; i < N; ++i) { ct[i] = cos(two_pi * i / N); st[i] = sin(two_pi * i / N); }
    for (int tt = 0; tt < g.W; ++tt) {
        const double w = 0.5 - 0.5 * cos(two_pi * tt / g.W);
        const int j = g.off + tt;
        const double sign = (j & 1) ? -1.0 : 1.0;      // cos(pi j)
        t->wsq[tt] = (float)(w * w);
        for (int k = 0; k < H; ++k) {
            const int idx = (int)(((int64_t)j * k) % N);
            float* p = &t->fb[(size_t)tt * g.ldb + (k / 32) * 64 + (k % 32)];
            p[0] = (float)(w * ct[idx]);
            p[32] = k == 0 ? (float)(w * sign) : (float)(-w * st[idx]);
            const double h = k == 0 ? 1.0 : 2.0;
            t->ib[(size_t)(2 * k) * g.ldi + tt] = (float)(w * h * ct[idx] / N);
            t->ib[(size_t)(2 * k + 1) * g.ldi + tt] = k == 0 ? (float)(w * sign / N) : (float)(-w * h * st[idx] / N);
        }
    }
}

// ---- validation: what every entry point runs before any device call
#define WN_GL_FAIL(code, ...) do { if (msg && cap > 0) snprintf(msg, (size_t)cap, __VA_ARGS__); return (code); } while (0)

static inline int wn_griffin_check_config(const wn_griffin_config* cfg, char* msg, int cap) {
    if (!cfg) WN_GL_FAIL(WN_E_ARG, "null configuration");
    if (cfg->abi_version != WN_ABI_VERSION) WN_GL_FAIL(WN_E_ARG, "abi_version %d != %d", cfg->abi_version, WN_ABI_VERSION);
    if (cfg->max_batch < 0 || cfg->max_frames < 0) WN_GL_FAIL(WN_E_ARG, "max_batch / max_frames must be >= 0");
    if (cfg->num_mels < 0 || cfg->num_mels > GL_MAX_MELS) WN_GL_FAIL(WN_E_ARG, "num_mels (%d) must be in [0, %d]", cfg->num_mels, GL_MAX_MELS);
    if (!(cfg->magnitude_power > 0.0f) || isinf(cfg->magnitude_power)) WN_GL_FAIL(WN_E_ARG, "magnitude_power (%g) must be finite and > 0", (double)cfg->magnitude_power);
    if (!(cfg->power > 0.0f) || isinf(cfg->power)) WN_GL_FAIL(WN_E_ARG, "power (%g) must be finite and > 0", (double)cfg->power);
    if (cfg->signal_normalization && (!(cfg->min_level_db < 0.0f) || !(cfg->max_abs_value > 0.0f)))
        WN_GL_FAIL(WN_E_ARG, "signal_normalization needs min_level_db (%g) < 0 and max_abs_value (%g) > 0", (double)cfg->min_level_db, (double)cfg->max_abs_value);
    if (cfg->n_fft < 8 || cfg->n_fft % 2) WN_GL_FAIL(WN_E_SHAPE, "n_fft (%d) must be even and >= 8", cfg->n_fft);
    if (cfg->win_size < 4 || cfg->win_size > cfg->n_fft) WN_GL_FAIL(WN_E_SHAPE, "win_size (%d) must be in [4, n_fft = %d]", cfg->win_size, cfg->n_fft);
    if (cfg->hop < 1 || cfg->hop > cfg->win_size / 4) WN_GL_FAIL(WN_E_SHAPE, "hop (%d) must be in [1, win_size / 4 = %d]", cfg->hop, cfg->win_size / 4);
    if (cfg->max_batch > 0 && cfg->max_frames < 2) WN_GL_FAIL(WN_E_SHAPE, "max_frames (%d) must be >= 2", cfg->max_frames);
    if (cfg->max_frames > 0 && (int64_t)cfg->hop * (cfg->max_frames - 1) > 0x7fffffffLL) WN_GL_FAIL(WN_E_SHAPE, "hop (max_frames - 1) must stay below 2^31");
    if (cfg->n_fft % 32 || cfg->n_fft > GL_MAX_FFT)
        WN_GL_FAIL(WN_E_UNSUPPORTED, "n_fft (%d) must be a multiple of 32 and <= %d: the products run in whole 32-column groups and a 32-frame tile's span must fit the LDS",
                   cfg->n_fft, GL_MAX_FFT);
    return WN_OK;
}
// kinds of `src`
#define GL_SRC_MEL 0           // [B, F_max, num_mels]
#define GL_SRC_MEL_CF 1        // [B, num_mels, F_max]
#define GL_SRC_MAG 2           // [B, F_max, 1 + n_fft / 2]
// a fresh run (not a continuation); max_batch < 0: no limit on B and the frames (the host hook)
static inline int wn_griffin_check_run(const char* who, const wn_griffin_config* cfg, int have_pinv, int32_t max_batch, const float* src, int32_t src_kind, int32_t F_max,
                                       const int32_t* frames, int32_t B, const float* y0, int64_t y0_pitch, int32_t iters, const float* out, int64_t out_pitch, char* msg, int cap) {
    if (!src || !frames) WN_GL_FAIL(WN_E_ARG, "%s: null argument", who);
    if (src_kind < 0 || src_kind > 2) WN_GL_FAIL(WN_E_ARG, "%s: src_kind (%d) must be 0 ... 2", who, src_kind);
    if (src_kind != GL_SRC_MAG && (!have_pinv || cfg->num_mels < 1)) WN_GL_FAIL(WN_E_ARG, "%s: a mel input needs num_mels >= 1 and the pseudo-inverse at create", who);
    if (B < 1) WN_GL_FAIL(WN_E_ARG, "%s: B (%d) must be >= 1", who, B);
    if (iters < 0) WN_GL_FAIL(WN_E_ARG, "%s: iters (%d) is negative", who, iters);
    if (y0_pitch < 0 || out_pitch < 0) WN_GL_FAIL(WN_E_ARG, "%s: a pitch is negative", who);
    if (max_batch >= 0 && B > max_batch) WN_GL_FAIL(WN_E_SHAPE, "%s: B (%d) > max_batch = %d", who, B, max_batch);
    for (int b = 0; b < B; ++b) {
        if (frames[b] < 2) WN_GL_FAIL(WN_E_SHAPE, "%s: frames[%d] = %d: a row needs at least 2 frames", who, b, frames[b]);
        if (frames[b] > F_max) WN_GL_FAIL(WN_E_SHAPE, "%s: frames[%d] = %d > F_max = %d", who, b, frames[b], F_max);
        if (max_batch >= 0 && frames[b] > cfg->max_frames) WN_GL_FAIL(WN_E_SHAPE, "%s: frames[%d] = %d exceeds max_frames = %d", who, b, frames[b], cfg->max_frames);
        const int64_t n = (int64_t)cfg->hop * (frames[b] - 1);
        if (n > 0x7fffffffLL) WN_GL_FAIL(WN_E_SHAPE, "%s: frames[%d] = %d gives more than 2^31 - 1 samples", who, b, frames[b]);
        if (y0 && n > y0_pitch) WN_GL_FAIL(WN_E_SHAPE, "%s: row %d has %lld samples > y0_pitch = %lld", who, b, (long long)n, (long long)y0_pitch);
        if (out && n > out_pitch) WN_GL_FAIL(WN_E_SHAPE, "%s: row %d has %lld samples > out_pitch = %lld", who, b, (long long)n, (long long)out_pitch);
    }
    return WN_OK;
}

// ---- host: the operation in plain float32 on the tables above, in the device's order: fused multiply-adds ascending in the device's interleaved chains
// (the forward sum in two, tap pair (t >> 1) & 1; the inverse sum in four, packed column pair (c >> 1) & 3), joined as the kernels join them
// X of frame f of a row y of n samples, packed: spec[2 k], spec[2 k + 1] = re, im of bin k (spec[1] = Re X[H]); spec holds 2 N floats (scratch behind N)
static inline void gl_host_analyse(const GlTables& t, const float* y, int64_t n, int64_t f, float* spec) {
#pragma clang fp contract(off)
    const GlGeom& g = t.g;
    const int N = g.N, H = g.H;
    const int64_t s0 = f * g.hop - g.Hl;
    for (int c = 0; c < 2 * N; ++c) spec[c] = 0.0f;
    for (int tt = 0; tt < g.W; ++tt) {
        const int64_t s = s0 + tt;
        if (s < 0 || s >= n) continue;      // a zero sample adds exactly nothing
        const float x = y[s];
        const float* row = &t.fb[(size_t)tt * g.ldb];
        float* acc = spec + ((tt >> 1) & 1) * N;
        for (int k = 0; k < H; ++k) {
            const float* p = row + (k / 32) * 64 + (k % 32);
            acc[2 * k] = __builtin_fmaf(x, p[0], acc[2 * k]);
            acc[2 * k + 1] = __builtin_fmaf(x, p[32], acc[2 * k + 1]);
        }
    }
    for (int c = 0; c < N; ++c) spec[c] = spec[c] + spec[N + c];
}
// a packed spectrum -> the frame's W windowed samples (fr [ldi]); ch: 4 ldi floats of scratch (the four chains of the inverse sum)
static inline void gl_host_synth(const GlTables& t, const float* spec, float* ch, float* fr) {
#pragma clang fp contract(off)
    const GlGeom& g = t.g;
    for (size_t e = 0; e < (size_t)4 * g.ldi; ++e) ch[e] = 0.0f;
    for (int c = 0; c < g.N; ++c) {
        const float v = spec[c];
        const float* row = &t.ib[(size_t)c * g.ldi];
        float* acc = &ch[(size_t)((c >> 1) & 3) * g.ldi];
        for (int j = 0; j < g.W; ++j) acc[j] = __builtin_fmaf(v, row[j], acc[j]);
    }
    for (int j = 0; j < g.ldi; ++j) fr[j] = (ch[j] + ch[g.ldi + j]) + (ch[2 * (size_t)g.ldi + j] + ch[3 * (size_t)g.ldi + j]);
}
// the frames fr [F][ldi] of a row -> its n = hop (F - 1) samples
static inline void gl_host_gather(const GlTables& t, const float* fr, int64_t F, float* y) {
#pragma clang fp contract(off)
    const GlGeom& g = t.g;
    const int64_t n = (int64_t)g.hop * (F - 1);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t p = i + g.Hl;
        const int64_t f_lo = p >= g.W ? (p - g.W) / g.hop + 1 : 0, f_hi = p / g.hop < F - 1 ? p / g.hop : F - 1;
        float num = 0.0f, den = 0.0f;
        for (int64_t f = f_lo; f <= f_hi; ++f) { const int64_t j = p - f * g.hop; num = num + fr[(size_t)f * g.ldi + j]; den = den + t.wsq[j]; }
        y[i] = num / den;
    }
}
// the projection of a packed spectrum in place on the magnitudes S [NB]
static inline void gl_host_project(const GlGeom& g, float* spec, const float* S) {
    spec[0] = gl_project_real(spec[0], S[0]);
    spec[1] = gl_project_real(spec[1], S[g.H]);
    for (int k = 1; k < g.H; ++k) gl_project(spec[2 * k], spec[2 * k + 1], S[k], &spec[2 * k], &spec[2 * k + 1]);
}
// the magnitudes mag [B][F_max][NB] of a call (frames beyond a row's keep what mag held)
static inline void gl_host_magnitudes(const wn_griffin_config& cfg, const float* pinvT, const float* src, int32_t src_kind, int32_t F_max, const int32_t* frames, int32_t B, float* mag) {
    const int NB = 1 + cfg.n_fft / 2, M = cfg.num_mels;
    const GlMelMap a = gl_mel_map(cfg);
    std::vector<float> amp((size_t)(M > 0 ? M : 1));
    for (int64_t b = 0; b < B; ++b)
        for (int64_t f = 0; f < frames[b]; ++f) {
            float* dst = mag + ((size_t)b * F_max + f) * NB;
            if (src_kind == GL_SRC_MAG) { for (int k = 0; k < NB; ++k) dst[k] = src[((size_t)b * F_max + f) * NB + k]; continue; }
            for (int m = 0; m < M; ++m) amp[m] = gl_mel_amp(a, src_kind == GL_SRC_MEL ? src[((size_t)b * F_max + f) * M + m] : src[((size_t)b * M + m) * F_max + f]);
            for (int k = 0; k < NB; ++k) dst[k] = gl_mel_bin(a, amp.data(), pinvT, NB, k);
        }
}
// one row: the start (y0, else u, else zero phase), then iters iterations; y [n]; pre (optional): the unpacked spectrum [F][NB][2] before the last projection
static inline void gl_host_row(const GlTables& t, const float* S, const float* u, const float* y0, int64_t F, int32_t iters, float* y, float* pre) {
    const GlGeom& g = t.g;
    const int N = g.N, H = g.H, NB = g.NB;
    const int64_t n = (int64_t)g.hop * (F - 1);
    std::vector<float> spec((size_t)2 * N), ch((size_t)4 * g.ldi), fr((size_t)F * g.ldi);
    if (y0) { for (int64_t i = 0; i < n; ++i) y[i] = y0[i]; }
    else {
        for (int64_t f = 0; f < F; ++f) {
            const float* Sf = S + (size_t)f * NB;
            const float* uf = u ? u + (size_t)f * NB : nullptr;
            float d;
            if (uf) { gl_start(Sf[0], uf[0], &spec[0], &d); gl_start(Sf[H], uf[H], &spec[1], &d); } else { spec[0] = Sf[0]; spec[1] = Sf[H]; }
            for (int k = 1; k < H; ++k) {
                if (uf) gl_start(Sf[k], uf[k], &spec[2 * k], &spec[2 * k + 1]); else { spec[2 * k] = Sf[k]; spec[2 * k + 1] = 0.0f; }
            }
            gl_host_synth(t, spec.data(), ch.data(), &fr[(size_t)f * g.ldi]);
        }
        gl_host_gather(t, fr.data(), F, y);
    }
    for (int it = 0; it < iters; ++it) {
        for (int64_t f = 0; f < F; ++f) {
            gl_host_analyse(t, y, n, f, spec.data());
            if (pre && it == iters - 1) {
                float* p = pre + (size_t)f * NB * 2;
                p[0] = spec[0]; p[1] = 0.0f; p[2 * H] = spec[1]; p[2 * H + 1] = 0.0f;
                for (int k = 1; k < H; ++k) { p[2 * k] = spec[2 * k]; p[2 * k + 1] = spec[2 * k + 1]; }
            }
            gl_host_project(g, spec.data(), S + (size_t)f * NB);
            gl_host_synth(t, spec.data(), ch.data(), &fr[(size_t)f * g.ldi]);
        }
        gl_host_gather(t, fr.data(), F, y);
    }
}
