// Reconstruction check arithmetic shared by the device kernels of wn_melcmp.hip, the host hook wn_test_melcmp_host and the stand-alone host program
// tests/host/melcmp_main.cpp: the difference of two mel elements, the per-frame distances over a frame's channels, one lane's share of a reduction
// over frames and the tree that joins the lanes, the DCT table, and the validation of a configuration and of a call.  Everything here is written once
// and runs on either side, so the hook gives the device's bits.
//
// Order of every sum (what "fixed order" means here):
//   over channels      m = 0 ... M - 1 ascending in one accumulator; the dot products of the cepstral distance by fused multiply-add;
//   over coefficients  lane group q of MELCMP_KQ = 4 takes k = 1 + q, 5 + q, ... ascending, and the four partial sums join as ((p0 + p1) + p2) + p3;
//   over frames        lane t of MELCMP_THREADS = 256 takes f = t, t + 256, ... ascending, and the 256 partial sums join in a halving tree
//                      (t += t + 128, t += t + 64, ...).
// None of them depends on anything but the row's own frame count.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/wavenet_mi355.h"

#define MELCMP_GROUP 32        // rows per launch
#define MELCMP_TF 64           // frames per tile (one wavefront's lanes)
#define MELCMP_KQ 4            // lane groups that share a frame's cepstral coefficients (the workgroup's four wavefronts)
#define MELCMP_THREADS 256     // = MELCMP_TF * MELCMP_KQ
#define MELCMP_MAX_MELS 128

// pitch (in floats) of one frame's channels in the LDS tile: odd, so that lanes on consecutive frames fall on distinct banks
__host__ __device__ __forceinline__ int melcmp_tile_pitch(int M) { return M | 1; }

// d = fl32(unit * fl32(a - b)): two roundings, never one fma
__host__ __device__ __forceinline__ float melcmp_diff(float unit, float a, float b) {
#pragma clang fp contract(off)
    const float e = a - b;
    return unit * e;
}

// one frame's channels d[0 ... M - 1]: the three sums of which bias, l1 and lsd are made
__host__ __device__ __forceinline__ float melcmp_frame_bias(const float* d, int M) {
#pragma clang fp contract(off)
    float s = 0.0f;
    for (int m = 0; m < M; ++m) s = s + d[m];
    return s / (float)M;
}
__host__ __device__ __forceinline__ float melcmp_frame_l1(const float* d, int M, float off) {
#pragma clang fp contract(off)
    float s = 0.0f;
    for (int m = 0; m < M; ++m) s = s + fabsf(d[m] - off);
    return s / (float)M;
}
__host__ __device__ __forceinline__ float melcmp_frame_lsd(const float* d, int M, float off) {
#pragma clang fp contract(off)
    float s = 0.0f;
    for (int m = 0; m < M; ++m) { const float e = d[m] - off; s = s + e * e; }
    return sqrtf(s / (float)M);
}
// lane group q's share of sum_k c_k^2; dct: rows k = 1 ... n_cep of D, [n_cep][M]
__host__ __device__ __forceinline__ float melcmp_frame_cep_part(const float* d, const float* dct, int M, int n_cep, int q) {
#pragma clang fp contract(off)
    float p = 0.0f;
    for (int k = 1 + q; k <= n_cep; k += MELCMP_KQ) {
        const float* row = dct + (size_t)(k - 1) * M;
        float c = 0.0f;
        for (int m = 0; m < M; ++m) c = __builtin_fmaf(row[m], d[m], c);
        p = p + c * c;
    }
    return p;
}
__host__ __device__ __forceinline__ float melcmp_frame_mcd(float p0, float p1, float p2, float p3) {
#pragma clang fp contract(off)
    const float s = ((p0 + p1) + p2) + p3;
    return sqrtf(0.5f * s);
}

// one lane's share of a sum over a row's n frames, and of the search for the worst frame
__host__ __device__ __forceinline__ float melcmp_lane_sum(const float* v, int n, int t) {
#pragma clang fp contract(off)
    float s = 0.0f;
    for (int f = t; f < n; f += MELCMP_THREADS) s = s + v[f];
    return s;
}
__host__ __device__ __forceinline__ void melcmp_lane_worst(const float* v, int n, int t, float alarm, float* worst, int32_t* at, int32_t* count) {
    float w = 0.0f; int32_t i = -1, c = 0;
    for (int f = t; f < n; f += MELCMP_THREADS) {
        const float x = v[f];
        if (i < 0 || x > w) { w = x; i = f; }
        c += x > alarm ? 1 : 0;
    }
    *worst = w; *at = i; *count = c;
}
// joining two lanes' candidates: the larger value, the earlier frame among equals (exact in any order)
__host__ __device__ __forceinline__ void melcmp_join_worst(float* w, int32_t* i, float w2, int32_t i2) {
    if (i2 >= 0 && (*i < 0 || w2 > *w || (w2 == *w && i2 < *i))) { *w = w2; *i = i2; }
}
__host__ __device__ __forceinline__ float melcmp_mean(float sum, int n) {
#pragma clang fp contract(off)
    return n > 0 ? sum / (float)n : 0.0f;
}

// ---- host: the table, one whole call in the device's order (the hook and melcmp_main.cpp), and the validation every entry point runs before any device call
// rows k = 1 ... n_cep of the orthonormal DCT-II, in double, rounded to float32: out [n_cep][M]
static inline void wn_melcmp_dct_table(int M, int n_cep, float* out) {
    const double pi = 3.14159265358979323846, s = sqrt(2.0 / (double)M);
    for (int k = 1; k <= n_cep; ++k)
        for (int m = 0; m < M; ++m) out[(size_t)(k - 1) * M + m] = (float)(s * cos(pi * (double)k * ((double)m + 0.5) / (double)M));
}

static inline float melcmp_host_tree(float* part) {
#pragma clang fp contract(off)
    for (int h = MELCMP_THREADS / 2; h > 0; h >>= 1)
        for (int t = 0; t < h; ++t) part[t] = part[t] + part[t + h];
    return part[0];
}
static inline float melcmp_host_row_sum(const float* v, int n) {
    float part[MELCMP_THREADS];
    for (int t = 0; t < MELCMP_THREADS; ++t) part[t] = melcmp_lane_sum(v, n, t);
    return melcmp_host_tree(part);
}
static inline float melcmp_host_at(const float* x, int cf, int64_t pitch, int M, int64_t row, int f, int m) {
    return cf ? x[(row * M + m) * pitch + f] : x[(row * pitch + f) * M + m];
}

// every row of a call; per_frame [B, 6, out_pitch] is required here (the hook passes a scratch when its caller passes none); dct from wn_melcmp_dct_table;
// col: scratch of M floats
static inline void wn_melcmp_host_rows(const wn_melcmp_config* cfg, const float* dct, const float* a, int a_cf, int64_t a_pitch, const float* b, int b_cf, int64_t b_pitch,
                                       const int32_t* frames, int32_t B, float* per_frame, int64_t out_pitch, float* summary, int32_t* marks, float* col) {
    const int M = cfg->num_mels;
    for (int64_t r = 0; r < B; ++r) {
        const int n = frames[r];
        float* pf = per_frame + r * 6 * out_pitch;
        float* sm = summary + r * 7;
        for (int f = 0; f < n; ++f) {
            for (int m = 0; m < M; ++m) col[m] = melcmp_diff(cfg->unit_db, melcmp_host_at(a, a_cf, a_pitch, M, r, f, m), melcmp_host_at(b, b_cf, b_pitch, M, r, f, m));
            pf[0 * out_pitch + f] = melcmp_frame_bias(col, M);
            pf[1 * out_pitch + f] = melcmp_frame_l1(col, M, 0.0f);
            pf[2 * out_pitch + f] = melcmp_frame_lsd(col, M, 0.0f);
            pf[3 * out_pitch + f] = melcmp_frame_mcd(melcmp_frame_cep_part(col, dct, M, cfg->n_cep, 0), melcmp_frame_cep_part(col, dct, M, cfg->n_cep, 1),
                                                     melcmp_frame_cep_part(col, dct, M, cfg->n_cep, 2), melcmp_frame_cep_part(col, dct, M, cfg->n_cep, 3));
        }
        for (int j = 0; j < 4; ++j) sm[j] = melcmp_mean(melcmp_host_row_sum(pf + j * out_pitch, n), n);
        const float off = sm[0];
        for (int f = 0; f < n; ++f) {
            for (int m = 0; m < M; ++m) col[m] = melcmp_diff(cfg->unit_db, melcmp_host_at(a, a_cf, a_pitch, M, r, f, m), melcmp_host_at(b, b_cf, b_pitch, M, r, f, m));
            pf[4 * out_pitch + f] = melcmp_frame_l1(col, M, off);
            pf[5 * out_pitch + f] = melcmp_frame_lsd(col, M, off);
        }
        for (int j = 4; j < 6; ++j) sm[j] = melcmp_mean(melcmp_host_row_sum(pf + j * out_pitch, n), n);
        float w = 0.0f; int32_t at = -1, count = 0;
        for (int t = 0; t < MELCMP_THREADS; ++t) {
            float w2; int32_t i2, c2;
            melcmp_lane_worst(pf + 4 * out_pitch, n, t, cfg->alarm_db, &w2, &i2, &c2);
            melcmp_join_worst(&w, &at, w2, i2);
            count += c2;
        }
        sm[6] = w; marks[r * 2] = at; marks[r * 2 + 1] = count;
    }
}

#define WN_MELCMP_FAIL(code, ...) do { if (msg && cap > 0) snprintf(msg, (size_t)cap, __VA_ARGS__); return (code); } while (0)

static inline int wn_melcmp_check_config(const wn_melcmp_config* cfg, char* msg, int cap) {
    if (!cfg) WN_MELCMP_FAIL(WN_E_ARG, "null configuration");
    if (cfg->abi_version != WN_ABI_VERSION) WN_MELCMP_FAIL(WN_E_ARG, "abi_version %d != %d", cfg->abi_version, WN_ABI_VERSION);
    if (cfg->num_mels < 1 || cfg->num_mels > MELCMP_MAX_MELS) WN_MELCMP_FAIL(WN_E_ARG, "num_mels (%d) must be 1 ... %d", cfg->num_mels, MELCMP_MAX_MELS);
    if (cfg->n_cep < 0 || cfg->n_cep > cfg->num_mels - 1) WN_MELCMP_FAIL(WN_E_ARG, "n_cep (%d) must be 0 ... num_mels - 1 = %d", cfg->n_cep, cfg->num_mels - 1);
    if (!(cfg->unit_db > 0.0f) || isinf(cfg->unit_db)) WN_MELCMP_FAIL(WN_E_ARG, "unit_db (%g) must be finite and > 0", (double)cfg->unit_db);
    if (!(cfg->alarm_db >= 0.0f) || isinf(cfg->alarm_db)) WN_MELCMP_FAIL(WN_E_ARG, "alarm_db (%g) must be finite and >= 0", (double)cfg->alarm_db);
    if (cfg->max_batch < 0) WN_MELCMP_FAIL(WN_E_ARG, "max_batch (%d) must be >= 0", cfg->max_batch);
    if (cfg->max_frames < 0) WN_MELCMP_FAIL(WN_E_ARG, "max_frames (%d) must be >= 0", cfg->max_frames);
    return WN_OK;
}
// one call of wn_melcmp_run; argument errors first, then shapes
static inline int wn_melcmp_check_call(const char* who, int32_t max_batch, int32_t max_frames, const float* a, int64_t a_pitch, const float* b, int64_t b_pitch, const int32_t* frames,
                                       int32_t B, const float* per_frame, int64_t out_pitch, const float* summary, const int32_t* marks, char* msg, int cap) {
    if (!a || !b || !frames || !summary || !marks) WN_MELCMP_FAIL(WN_E_ARG, "%s: null argument", who);
    if (B < 1) WN_MELCMP_FAIL(WN_E_ARG, "%s: B (%d) must be >= 1", who, B);
    int32_t n_max = 0;
    for (int r = 0; r < B; ++r) {
        if (frames[r] < 0) WN_MELCMP_FAIL(WN_E_ARG, "%s: frames[%d] = %d is negative", who, r, frames[r]);
        if (frames[r] > n_max) n_max = frames[r];
    }
    if (B > max_batch) WN_MELCMP_FAIL(WN_E_SHAPE, "%s: B (%d) > max_batch = %d", who, B, max_batch);
    if (n_max > max_frames) WN_MELCMP_FAIL(WN_E_SHAPE, "%s: the longest row (%d frames) > max_frames = %d", who, n_max, max_frames);
    if (a_pitch < n_max) WN_MELCMP_FAIL(WN_E_SHAPE, "%s: a_pitch (%lld) < the longest row (%d)", who, (long long)a_pitch, n_max);
    if (b_pitch < n_max) WN_MELCMP_FAIL(WN_E_SHAPE, "%s: b_pitch (%lld) < the longest row (%d)", who, (long long)b_pitch, n_max);
    if (per_frame && out_pitch < n_max) WN_MELCMP_FAIL(WN_E_SHAPE, "%s: out_pitch (%lld) < the longest row (%d)", who, (long long)out_pitch, n_max);
    return WN_OK;
}
