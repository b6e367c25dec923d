// Pitch check arithmetic shared by the device kernels of wn_pitch.hip, the host hooks wn_test_pitch_host / wn_test_pitch_compare_host and the stand-alone
// host program tests/host/pitch_main.cpp: one term of the difference function, the normalisation of a frame's lags, the pick with its parabolic
// refinement, one frame's share of a comparison and the sums that join the frames, and the validation of a configuration and of a call.  Everything
// here is written once and runs on either side, so the hooks give the device's bits (the comparison's log2 in double is the one library call whose last
// bit may differ between the two sides).
//
// The estimator is YIN (de Cheveigne & Kawahara 2002, steps 2 ... 5) on frames aligned with the mel frames.  With L = window + tau_max, frame f covers the
// signal indices [f hop - L / 2, f hop - L / 2 + L), zeros outside [0, n); call them x_0 ... x_{L-1}.
//   d(tau)  = sum_{j = 0 ... W-1} (x_j - x_{j+tau})^2     tau = 1 ... tau_max; one float32 accumulator, j ascending, e = x_j - x_{j+tau}; acc = fma(e, e, acc)
//   c(tau)  = sum_{k = 1 ... tau} d(k)                     float32, tau ascending, sequential
//   d'(0)   = 1;  d'(tau) = c(tau) > 0 ? (d(tau) tau) / c(tau) : 1
// The direct form of d on purpose: every term is non-negative, so d -- and with it c and d' -- has a RELATIVE error bound, (W + tau_max + 8) 2^-24; the
// energy-minus-autocorrelation form cancels and has none.  Pick over tau in [tau_min, tau_max - 1]: the first tau with d'(tau) < threshold, then walk while
// tau + 1 <= tau_max - 1 and d'(tau + 1) < d'(tau).  Found: voiced, f0 = sample_rate / (tau + delta) with the parabola through d'(tau - 1), d'(tau), d'(tau + 1),
// ap = d'(tau).  Not found: f0 = 0, ap = the minimum of d' over the range.  No energy gate, no smoothing, no octave post-processing.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/wavenet_mi355.h"

#define PITCH_THREADS 256      // lanes of a workgroup: each owns lags
#define PITCH_TILE 8           // frames per workgroup (wn_pitch_frame_tile)
#define PITCH_CHAINS 4         // (frame, lag) accumulator chains a lane runs side by side: frames 4 g ... 4 g + 3 of the tile at one lag
#define PITCH_GROUP 64         // rows per launch: their lengths travel as kernel arguments
#define PITCH_LDS_FLOATS 16384 // the LDS the kernel is built for, 64 KiB: the tile's signal span and its d' table
#define PITCH_COLS 9           // frames, voiced_a, voiced_b, both, vuv_error, gpe, f0_rmse_cents, f0_bias_cents, f0_fine_rmse_cents

// floats of one tile's signal span, padded to whole 16-byte slots, and of the whole tile in LDS
__host__ __device__ __forceinline__ int64_t pitch_span_floats(int64_t hop, int64_t window, int64_t tau_max) {
    return ((PITCH_TILE - 1) * hop + window + tau_max + 3) & ~(int64_t)3;
}
__host__ __device__ __forceinline__ int64_t pitch_lds_floats(int64_t hop, int64_t window, int64_t tau_max) {
    return pitch_span_floats(hop, window, tau_max) + PITCH_TILE * (tau_max + 1);
}

// one term of d: two roundings (the difference, then the fused multiply-add)
__host__ __device__ __forceinline__ float pitch_term(float acc, float xj, float xjt) {
#pragma clang fp contract(off)
    const float e = xj - xjt;
    return __builtin_fmaf(e, e, acc);
}

// d[1 ... tau_max] of one frame -> d'[0 ... tau_max] in place
__host__ __device__ __forceinline__ void pitch_normalise(float* d, int tau_max) {
#pragma clang fp contract(off)
    float c = 0.0f;
    d[0] = 1.0f;
    for (int tau = 1; tau <= tau_max; ++tau) {
        const float v = d[tau];
        c = c + v;
        d[tau] = c > 0.0f ? (v * (float)tau) / c : 1.0f;
    }
}

// the pick and the frame's two outputs from d'[0 ... tau_max]
__host__ __device__ __forceinline__ void pitch_pick(const float* dp, int tau_min, int tau_max, float threshold, float sample_rate, float* f0, float* ap) {
#pragma clang fp contract(off)
    int at = -1;
    float low = dp[tau_min];
    for (int tau = tau_min; tau <= tau_max - 1; ++tau) {
        const float v = dp[tau];
        if (v < threshold) { at = tau; break; }
        low = v < low ? v : low;
    }
    if (at < 0) { *f0 = 0.0f; *ap = low; return; }
    while (at + 1 <= tau_max - 1 && dp[at + 1] < dp[at]) ++at;
    const float a = dp[at - 1], b = dp[at], c = dp[at + 1];
    const float den = (a - 2.0f * b) + c;
    const float delta = den > 0.0f ? (0.5f * (a - c)) / den : 0.0f;
    *f0 = sample_rate / ((float)at + delta);
    *ap = b;
}

// ---- comparison of two f0 tracks: what one frame contributes, and the sums in frame order
struct PitchCmpSums { int32_t va = 0, vb = 0, both = 0, differ = 0, gross = 0; double s1 = 0.0, s2 = 0.0, s2_fine = 0.0; };

// flags: bit 0 a voiced, bit 1 b voiced, bit 2 gross (both voiced and |f_b / f_a - 1| > 0.2); cents = 1200 log2(f_b / f_a) in double for a both-voiced frame, else 0
__host__ __device__ __forceinline__ void pitch_cmp_frame(float fa, float fb, int32_t* flags, double* cents) {
    const int va = fa > 0.0f, vb = fb > 0.0f;
    int fl = va | (vb << 1);
    double ct = 0.0;
    if (va && vb) {
        const double r = (double)fb / (double)fa;
        ct = 1200.0 * log2(r);
        if (fabs(r - 1.0) > 0.2) fl |= 4;
    }
    *flags = fl; *cents = ct;
}
__host__ __device__ __forceinline__ void pitch_cmp_add(PitchCmpSums* s, int32_t flags, double cents) {
#pragma clang fp contract(off)
    const int va = flags & 1, vb = (flags >> 1) & 1;
    s->va += va; s->vb += vb; s->differ += va != vb;
    if (va && vb) {
        s->both += 1;
        s->s1 = s->s1 + cents;
        s->s2 = s->s2 + cents * cents;
        if (flags & 4) s->gross += 1;
        else s->s2_fine = s->s2_fine + cents * cents;
    }
}
__host__ __device__ __forceinline__ void pitch_cmp_finish(const PitchCmpSums* s, int32_t n, float* row) {
    const int32_t fine = s->both - s->gross;
    row[0] = (float)n; row[1] = (float)s->va; row[2] = (float)s->vb; row[3] = (float)s->both;
    row[4] = n > 0 ? (float)((double)s->differ / (double)n) : 0.0f;
    row[5] = s->both > 0 ? (float)((double)s->gross / (double)s->both) : 0.0f;
    row[6] = s->both > 0 ? (float)sqrt(s->s2 / (double)s->both) : 0.0f;
    row[7] = s->both > 0 ? (float)(s->s1 / (double)s->both) : 0.0f;
    row[8] = fine > 0 ? (float)sqrt(s->s2_fine / (double)fine) : 0.0f;
}

// ---- host: whole calls in the device's order (the hooks and pitch_main.cpp), and the validation every entry point runs before any device call
// x: scratch of window + tau_max floats, dp: scratch of tau_max + 1 floats.  Reads wav[b * ld + s] for 0 <= s < lengths[b] only; writes frames f < 1 + lengths[b] / hop only.
static inline void wn_pitch_host_rows(const wn_pitch_config* cfg, const float* wav, int64_t ld, const int32_t* lengths, int32_t B, int32_t F_max, float* f0, float* ap,
                                      float* dprime, float* x, float* dp) {
    const int W = cfg->window, TM = cfg->tau_max, L = W + TM;
    for (int64_t b = 0; b < B; ++b) {
        const int64_t n = lengths[b];
        const int64_t F = 1 + n / cfg->hop;
        for (int64_t f = 0; f < F; ++f) {
            const int64_t s0 = f * cfg->hop - L / 2;
            for (int i = 0; i < L; ++i) { const int64_t s = s0 + i; x[i] = s >= 0 && s < n ? wav[b * ld + s] : 0.0f; }
            for (int tau = 1; tau <= TM; ++tau) {
                float acc = 0.0f;
                for (int j = 0; j < W; ++j) acc = pitch_term(acc, x[j], x[j + tau]);
                dp[tau] = acc;
            }
            pitch_normalise(dp, TM);
            float v0, v1;
            pitch_pick(dp, cfg->tau_min, TM, cfg->threshold, (float)cfg->sample_rate, &v0, &v1);
            f0[b * F_max + f] = v0;
            if (ap) ap[b * F_max + f] = v1;
            if (dprime) for (int tau = 0; tau <= TM; ++tau) dprime[(b * F_max + f) * (TM + 1) + tau] = dp[tau];
        }
    }
}
static inline void wn_pitch_compare_host_rows(const float* f0_a, const float* f0_b, int64_t pitch, const int32_t* frames, int32_t B, float* table) {
    for (int64_t b = 0; b < B; ++b) {
        PitchCmpSums s;
        for (int64_t f = 0; f < frames[b]; ++f) {
            int32_t fl; double ct;
            pitch_cmp_frame(f0_a[b * pitch + f], f0_b[b * pitch + f], &fl, &ct);
            pitch_cmp_add(&s, fl, ct);
        }
        pitch_cmp_finish(&s, frames[b], table + b * PITCH_COLS);
    }
}

#define WN_PITCH_FAIL(code, ...) do { if (msg && cap > 0) snprintf(msg, (size_t)cap, __VA_ARGS__); return (code); } while (0)

static inline int wn_pitch_check_config(const wn_pitch_config* cfg, char* msg, int cap) {
    if (!cfg) WN_PITCH_FAIL(WN_E_ARG, "null configuration");
    if (cfg->abi_version != WN_ABI_VERSION) WN_PITCH_FAIL(WN_E_ARG, "abi_version %d != %d", cfg->abi_version, WN_ABI_VERSION);
    if (cfg->sample_rate < 1) WN_PITCH_FAIL(WN_E_ARG, "sample_rate (%d) must be >= 1", cfg->sample_rate);
    if (cfg->hop < 1) WN_PITCH_FAIL(WN_E_ARG, "hop (%d) must be >= 1", cfg->hop);
    if (cfg->window < 1) WN_PITCH_FAIL(WN_E_ARG, "window (%d) must be >= 1", cfg->window);
    if (cfg->tau_min < 2) WN_PITCH_FAIL(WN_E_ARG, "tau_min (%d) must be >= 2", cfg->tau_min);
    if ((int64_t)cfg->tau_max <= (int64_t)cfg->tau_min + 1) WN_PITCH_FAIL(WN_E_ARG, "tau_max (%d) must be > tau_min + 1 = %d", cfg->tau_max, cfg->tau_min + 1);
    if (!(cfg->threshold > 0.0f && cfg->threshold <= 1.0f)) WN_PITCH_FAIL(WN_E_ARG, "threshold (%g) must be in (0, 1]", (double)cfg->threshold);
    if (cfg->max_batch < 1) WN_PITCH_FAIL(WN_E_ARG, "max_batch (%d) must be >= 1", cfg->max_batch);
    if (cfg->max_samples < 0) WN_PITCH_FAIL(WN_E_ARG, "max_samples (%lld) must be >= 0", (long long)cfg->max_samples);
    if (cfg->max_samples > INT32_MAX) WN_PITCH_FAIL(WN_E_ARG, "max_samples (%lld) must be <= %d", (long long)cfg->max_samples, INT32_MAX);
    if (pitch_lds_floats(cfg->hop, cfg->window, cfg->tau_max) > PITCH_LDS_FLOATS)
        WN_PITCH_FAIL(WN_E_UNSUPPORTED, "a tile of %d frames needs %lld floats of LDS (7 hop + window + tau_max, and 8 (tau_max + 1)); the kernel is built for %d",
                      PITCH_TILE, (long long)pitch_lds_floats(cfg->hop, cfg->window, cfg->tau_max), PITCH_LDS_FLOATS);
    return WN_OK;
}
// one call of wn_pitch_run; argument errors first, then shapes
static inline int wn_pitch_check_run(const char* who, const wn_pitch_config* cfg, const float* wav, int64_t ld, const int32_t* lengths, int32_t B, int32_t F_max, const float* f0,
                                     char* msg, int cap) {
    if (!wav || !lengths || !f0) WN_PITCH_FAIL(WN_E_ARG, "%s: null argument", who);
    if (B < 1) WN_PITCH_FAIL(WN_E_ARG, "%s: B (%d) must be >= 1", who, B);
    if (F_max < 0) WN_PITCH_FAIL(WN_E_ARG, "%s: F_max (%d) is negative", who, F_max);
    if (ld < 0) WN_PITCH_FAIL(WN_E_ARG, "%s: ld (%lld) is negative", who, (long long)ld);
    if (B > cfg->max_batch) WN_PITCH_FAIL(WN_E_SHAPE, "%s: B (%d) > max_batch = %d", who, B, cfg->max_batch);
    for (int b = 0; b < B; ++b)
        if (lengths[b] < 0) WN_PITCH_FAIL(WN_E_ARG, "%s: lengths[%d] = %d is negative", who, b, lengths[b]);
    if ((int64_t)F_max > 1 + cfg->max_samples / cfg->hop)
        WN_PITCH_FAIL(WN_E_SHAPE, "%s: F_max (%d) > the %lld frames of max_samples = %lld", who, F_max, (long long)(1 + cfg->max_samples / cfg->hop), (long long)cfg->max_samples);
    for (int b = 0; b < B; ++b) {
        if (lengths[b] > ld) WN_PITCH_FAIL(WN_E_SHAPE, "%s: lengths[%d] = %d must be in [0, ld = %lld]", who, b, lengths[b], (long long)ld);
        if (lengths[b] > cfg->max_samples) WN_PITCH_FAIL(WN_E_SHAPE, "%s: lengths[%d] = %d exceeds max_samples = %lld", who, b, lengths[b], (long long)cfg->max_samples);
        if (F_max < 1 + lengths[b] / cfg->hop) WN_PITCH_FAIL(WN_E_SHAPE, "%s: F_max (%d) < the %d frames of lengths[%d] = %d", who, F_max, 1 + lengths[b] / cfg->hop, b, lengths[b]);
    }
    return WN_OK;
}
// one call of wn_pitch_compare; max_batch / max_frames < 0: no limit (the host hook)
static inline int wn_pitch_check_compare(const char* who, int32_t max_batch, int64_t max_frames, const float* f0_a, const float* f0_b, int64_t pitch, const int32_t* frames, int32_t B,
                                         const float* table, char* msg, int cap) {
    if (!f0_a || !f0_b || !frames || !table) WN_PITCH_FAIL(WN_E_ARG, "%s: null argument", who);
    if (B < 1) WN_PITCH_FAIL(WN_E_ARG, "%s: B (%d) must be >= 1", who, B);
    if (pitch < 0) WN_PITCH_FAIL(WN_E_ARG, "%s: pitch (%lld) is negative", who, (long long)pitch);
    for (int b = 0; b < B; ++b)
        if (frames[b] < 0) WN_PITCH_FAIL(WN_E_ARG, "%s: frames[%d] = %d is negative", who, b, frames[b]);
    if (max_batch >= 0 && B > max_batch) WN_PITCH_FAIL(WN_E_SHAPE, "%s: B (%d) > max_batch = %d", who, B, max_batch);
    for (int b = 0; b < B; ++b) {
        if (frames[b] > pitch) WN_PITCH_FAIL(WN_E_SHAPE, "%s: frames[%d] = %d > pitch = %lld", who, b, frames[b], (long long)pitch);
        if (max_frames >= 0 && frames[b] > max_frames) WN_PITCH_FAIL(WN_E_SHAPE, "%s: frames[%d] = %d > the %lld frames of max_samples", who, b, frames[b], (long long)max_frames);
    }
    return WN_OK;
}
