// Sample-rate conversion by a rational factor L / M: what the device code of wn_resample.hip, the host hooks wn_test_resample_host / wn_test_resample_table
// and the stand-alone host program tests/host/resample_main.cpp share -- the validation, the integer plan (L, M, W, T, n_out, the emit rule), the coefficient
// table in double rounded once to float32, the one-output arithmetic, and the whole state machine of a push on host arrays.
//
// g = gcd(sr_in, sr_out), L = sr_out / g, M = sr_in / g, s = min(1, L / M).  Prototype: h(t) = rolloff sinc(rolloff t) I0(beta sqrt(1 - (t / Z)^2)) / I0(beta) for
// |t| < Z, else 0 (a Kaiser-windowed sinc; the defaults are resampy's published kaiser_best values).  Output m of a row of n samples:
//   y[m] = s sum_k x[k] h(s (m M / L - k)),  x = 0 outside [0, n),  m < n_out = ceil(n L / M)
// and in polyphase form, with W = ceil(Z max(L, M) / L), T = 2 W, k0 = floor(m M / L), p = (m M) mod L:
//   y[m] = sum_{j < T} C[p][j] x[k0 - W + 1 + j],  C[p][j] = s h(s (p / L + W - 1 - j)) = s h((p + (W - 1 - j) L) / max(L, M))
// One float32 accumulator from 0, T fmaf in ascending j, taps outside the row read 0.0f and are never skipped: an output's bits depend on the table, m and the
// row's samples alone.  L = M = 1 does not filter: W = T = 0 and y[m] = x[m], the bits copied.
// A row since its restart: S samples given, E emitted.  Final: E = ceil(S L / M).  Otherwise E = max(0, ceil((S - W) L / M)): output m is emitted once its last
// tap k0 + W lies below S.  What a row carries: the inputs [lo(E), S), lo(E) = max(0, floor(E M / L) - W + 1), at most 2 W - 1 of them.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <vector>

#include "../../include/wavenet_mi355.h"

#define RS_MAX_TABLE_FLOATS (4LL << 20)      // L x T
#define RS_MAX_SPAN_FLOATS 12288             // the staged inputs of the smallest output block (48 KiB of LDS)
#define RS_MAX_BETA 256.0                    // I0(beta) stays far inside double
#define RS_THREADS 256
#define RS_PER_THREAD 4
#define RS_MIN_BLOCK 64                      // output blocks of 64 ... RS_THREADS * RS_PER_THREAD outputs

struct RsPlan { int64_t L = 1, M = 1, W = 0, T = 0; int32_t block = RS_THREADS * RS_PER_THREAD, span = 0; };

__host__ __device__ __forceinline__ int64_t rs_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }      // a >= 0, b > 0
__host__ __device__ __forceinline__ int64_t rs_num_out(int64_t n, int64_t L, int64_t M) { return rs_cdiv(n * L, M); }
__host__ __device__ __forceinline__ int64_t rs_ready(int64_t S, int64_t L, int64_t M, int64_t W, int final) {
    if (final) return rs_cdiv(S * L, M);
    return S > W ? rs_cdiv((S - W) * L, M) : 0;
}
// the first input the outputs from E on still read
__host__ __device__ __forceinline__ int64_t rs_tail_lo(int64_t E, int64_t L, int64_t M, int64_t W) {
    if (W == 0) return E;      // L = M = 1: nothing is carried
    const int64_t lo = E * M / L - W + 1;
    return lo > 0 ? lo : 0;
}
static inline int64_t rs_tail_cap(int64_t W) { return 2 * W + 2; }
// staged inputs of a block of `block` outputs: k0 moves by at most floor((block - 1) M / L) + 1 inside it
static inline int64_t rs_span_floats(int64_t block, int64_t L, int64_t M, int64_t W) { return (block - 1) * M / L + 2 + 2 * W; }

#define WN_RS_FAIL(code, ...) do { if (msg && cap > 0) snprintf(msg, (size_t)cap, __VA_ARGS__); return (code); } while (0)

static inline int64_t rs_gcd(int64_t a, int64_t b) { while (b) { const int64_t t = a % b; a = b; b = t; } return a; }

// validates a configuration and fills the plan
static inline int rs_check_config(const wn_resample_config* cfg, RsPlan* plan, char* msg, int cap) {
    if (!cfg) WN_RS_FAIL(WN_E_ARG, "null configuration");
    if (cfg->abi_version != WN_ABI_VERSION) WN_RS_FAIL(WN_E_ARG, "abi_version %d != %d", cfg->abi_version, WN_ABI_VERSION);
    if (cfg->max_rows < 0) WN_RS_FAIL(WN_E_ARG, "max_rows (%d) is negative", cfg->max_rows);
    if (cfg->max_in < 0) WN_RS_FAIL(WN_E_ARG, "max_in (%d) is negative", cfg->max_in);
    if (cfg->max_rows > 0 && cfg->max_in < 1) WN_RS_FAIL(WN_E_ARG, "max_in (%d) must be >= 1 on a handle with rows", cfg->max_in);
    if (cfg->sr_in < 1) WN_RS_FAIL(WN_E_ARG, "sr_in (%d) must be >= 1", cfg->sr_in);
    if (cfg->sr_out < 1) WN_RS_FAIL(WN_E_ARG, "sr_out (%d) must be >= 1", cfg->sr_out);
    if (cfg->zeros < 1) WN_RS_FAIL(WN_E_ARG, "zeros (%d) must be >= 1", cfg->zeros);
    if (!(cfg->rolloff > 0.0 && cfg->rolloff <= 1.0)) WN_RS_FAIL(WN_E_ARG, "rolloff (%g) must be in (0, 1]", cfg->rolloff);
    if (!(cfg->beta >= 0.0) || isinf(cfg->beta)) WN_RS_FAIL(WN_E_ARG, "beta (%g) must be finite and >= 0", cfg->beta);
    if (cfg->beta > RS_MAX_BETA) WN_RS_FAIL(WN_E_UNSUPPORTED, "beta (%g) is above the limit of %g", cfg->beta, RS_MAX_BETA);
    RsPlan p;
    const int64_t g = rs_gcd(cfg->sr_in, cfg->sr_out);
    p.L = cfg->sr_out / g; p.M = cfg->sr_in / g;
    if (p.L == 1 && p.M == 1) { p.W = 0; p.T = 0; p.span = 0; if (plan) *plan = p; return WN_OK; }
    const int64_t big = p.L > p.M ? p.L : p.M;
    p.W = rs_cdiv((int64_t)cfg->zeros * big, p.L); p.T = 2 * p.W;
    if ((double)p.L * (double)p.T > (double)RS_MAX_TABLE_FLOATS)
        WN_RS_FAIL(WN_E_UNSUPPORTED, "%d -> %d Hz with %d zero crossings needs a table of L x T = %lld x %lld floats, above the limit of %lld", cfg->sr_in, cfg->sr_out,
                   cfg->zeros, (long long)p.L, (long long)p.T, (long long)RS_MAX_TABLE_FLOATS);
    int64_t block = RS_THREADS * RS_PER_THREAD;
    while (block > RS_MIN_BLOCK && rs_span_floats(block, p.L, p.M, p.W) > RS_MAX_SPAN_FLOATS) block /= 2;
    if (rs_span_floats(block, p.L, p.M, p.W) > RS_MAX_SPAN_FLOATS)
        WN_RS_FAIL(WN_E_UNSUPPORTED, "%d -> %d Hz with %d zero crossings reads %lld inputs per block of %d outputs, above the limit of %d", cfg->sr_in, cfg->sr_out, cfg->zeros,
                   (long long)rs_span_floats(block, p.L, p.M, p.W), (int)block, RS_MAX_SPAN_FLOATS);
    p.block = (int32_t)block; p.span = (int32_t)rs_span_floats(block, p.L, p.M, p.W);
    if (plan) *plan = p;
    return WN_OK;
}

// ---- the coefficient table, in double on the host
static inline double rs_i0(double x) {      // sum_k ((x / 2)^k / k!)^2
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 2000; ++k) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-18 * sum) break;
    }
    return sum;
}
static inline double rs_sinc(double x) {
    if (x == 0.0) return 1.0;
    const double a = 3.14159265358979323846 * x;
    return sin(a) / a;
}
static inline double rs_proto(double t, int zeros, double beta, double rolloff, double i0_beta) {
    const double r = t / (double)zeros;
    if (!(fabs(r) < 1.0)) return 0.0;
    return rolloff * rs_sinc(rolloff * t) * rs_i0(beta * sqrt(1.0 - r * r)) / i0_beta;
}
// C [L][T], each entry evaluated in double at its own polyphase position and rounded once
static inline void rs_build_table(const wn_resample_config& cfg, const RsPlan& p, std::vector<float>* C) {
    C->assign((size_t)(p.L * p.T), 0.0f);
    const double big = (double)(p.L > p.M ? p.L : p.M), s = (double)p.L / big, i0b = rs_i0(cfg.beta);
    for (int64_t ph = 0; ph < p.L; ++ph)
        for (int64_t j = 0; j < p.T; ++j) {
            const double t = (double)(ph + (p.W - 1 - j) * p.L) / big;
            (*C)[(size_t)(ph * p.T + j)] = (float)(s * rs_proto(t, cfg.zeros, cfg.beta, cfg.rolloff, i0b));
        }
}

// ---- one output: T fmaf in ascending j from 0.0f.  x: the row's samples with x[0] the input `base`; inputs outside [0, S_end) read 0.0f
static inline float rs_host_output(const RsPlan& p, const float* C, const float* x, int64_t base, int64_t S_end, int64_t m) {
    const int64_t k0 = m * p.M / p.L, ph = m * p.M % p.L;
    if (p.T == 0) return x[m - base];
    const float* c = C + ph * p.T;
    float acc = 0.0f;
    for (int64_t j = 0; j < p.T; ++j) {
        const int64_t k = k0 - p.W + 1 + j;
        acc = fmaf(c[j], (k >= 0 && k < S_end) ? x[k - base] : 0.0f, acc);
    }
    return acc;
}
// a whole row
static inline void rs_host_row(const RsPlan& p, const float* C, const float* x, int64_t n, float* out) {
    const int64_t n_out = rs_num_out(n, p.L, p.M);
    for (int64_t m = 0; m < n_out; ++m) out[m] = rs_host_output(p, C, x, 0, n, m);
}

// ---- calls
static inline int rs_check_run(const char* who, const wn_resample_config& cfg, const RsPlan& p, int32_t max_rows, const float* in, int64_t in_pitch, const int32_t* lengths,
                               int32_t B, const float* out, int64_t out_pitch, char* msg, int cap) {
    if (!lengths || !out) WN_RS_FAIL(WN_E_ARG, "%s: null argument", who);
    if (B < 1) WN_RS_FAIL(WN_E_ARG, "%s: B (%d) must be >= 1", who, B);
    if (max_rows >= 0 && B > max_rows) WN_RS_FAIL(WN_E_SHAPE, "%s: B (%d) > max_rows = %d", who, B, max_rows);      // (before any of the B entries is read)
    if (in_pitch < 0) WN_RS_FAIL(WN_E_ARG, "%s: in_pitch (%lld) is negative", who, (long long)in_pitch);
    if (out_pitch < 0) WN_RS_FAIL(WN_E_ARG, "%s: out_pitch (%lld) is negative", who, (long long)out_pitch);
    int64_t n_max = 0;
    for (int b = 0; b < B; ++b) {
        if (lengths[b] < 0) WN_RS_FAIL(WN_E_ARG, "%s: lengths[%d] = %d is negative", who, b, lengths[b]);
        if (lengths[b] > n_max) n_max = lengths[b];
    }
    if (n_max > 0 && !in) WN_RS_FAIL(WN_E_ARG, "%s: null argument (in)", who);
    for (int b = 0; b < B; ++b)
        if (cfg.max_in > 0 && lengths[b] > cfg.max_in) WN_RS_FAIL(WN_E_SHAPE, "%s: lengths[%d] = %d > max_in = %d", who, b, lengths[b], cfg.max_in);
    if (in_pitch < n_max) WN_RS_FAIL(WN_E_SHAPE, "%s: in_pitch (%lld) < the longest row (%lld)", who, (long long)in_pitch, (long long)n_max);
    if (out_pitch < rs_num_out(n_max, p.L, p.M))
        WN_RS_FAIL(WN_E_SHAPE, "%s: out_pitch (%lld) < the longest row's outputs (%lld)", who, (long long)out_pitch, (long long)rs_num_out(n_max, p.L, p.M));
    return WN_OK;
}

struct RsRow { int64_t S = 0; bool ended = false; uint8_t par = 0; };      // par: the tail half the next push reads
struct RsStep { int64_t S0, S1, E0, E1; int32_t n; uint8_t active, final, par; };

// validates a push and plans every row; changes nothing.  max_rows < 0: no limit on B (the host hook)
static inline int rs_plan_push(const char* who, const wn_resample_config& cfg, const RsPlan& p, int32_t max_rows, const RsRow* rows, const float* in, int64_t in_pitch,
                               const int32_t* n, const int32_t* restart, const int32_t* final, int32_t B, const float* out, int64_t out_pitch, const int32_t* n_out, RsStep* steps,
                               char* msg, int cap) {
    if (!n || !out || !n_out) WN_RS_FAIL(WN_E_ARG, "%s: null argument", who);
    if (B < 1) WN_RS_FAIL(WN_E_ARG, "%s: B (%d) must be >= 1", who, B);
    if (max_rows >= 0 && B > max_rows) WN_RS_FAIL(WN_E_SHAPE, "%s: B (%d) > max_rows = %d", who, B, max_rows);      // (before any of the B entries is read)
    if (in_pitch < 0) WN_RS_FAIL(WN_E_ARG, "%s: in_pitch (%lld) is negative", who, (long long)in_pitch);
    if (out_pitch < 0) WN_RS_FAIL(WN_E_ARG, "%s: out_pitch (%lld) is negative", who, (long long)out_pitch);
    bool any = false;
    for (int b = 0; b < B; ++b) {
        if (n[b] < 0) WN_RS_FAIL(WN_E_ARG, "%s: n[%d] = %d is negative", who, b, n[b]);
        any = any || n[b] > 0;
    }
    if (any && !in) WN_RS_FAIL(WN_E_ARG, "%s: null argument (in)", who);
    for (int b = 0; b < B; ++b) {
        if (cfg.max_in > 0 && n[b] > cfg.max_in) WN_RS_FAIL(WN_E_SHAPE, "%s: n[%d] = %d > max_in = %d", who, b, n[b], cfg.max_in);
        if (n[b] > in_pitch) WN_RS_FAIL(WN_E_SHAPE, "%s: n[%d] = %d > in_pitch = %lld", who, b, n[b], (long long)in_pitch);
    }
    for (int b = 0; b < B; ++b) {
        RsStep& s = steps[b];
        const bool rs = restart && restart[b], fin = final && final[b];
        s.n = n[b]; s.final = fin; s.active = n[b] > 0 || fin; s.par = rows[b].par;
        if (s.active && rows[b].ended && !rs) WN_RS_FAIL(WN_E_STATE, "%s: row %d has ended (final): restart[%d] must be set on its next push", who, b, b);
        s.S0 = rs ? 0 : rows[b].S;
        s.S1 = s.S0 + n[b];
        if (s.S1 > 0x7fffffffLL) WN_RS_FAIL(WN_E_SHAPE, "%s: row %d would hold %lld samples since its restart, above 2^31 - 1", who, b, (long long)s.S1);
        s.E0 = rs_ready(s.S0, p.L, p.M, p.W, 0);
        s.E1 = s.active ? rs_ready(s.S1, p.L, p.M, p.W, fin) : s.E0;
        if (s.E1 - s.E0 > out_pitch) WN_RS_FAIL(WN_E_SHAPE, "%s: out_pitch (%lld) < n_out[%d] = %lld", who, (long long)out_pitch, b, (long long)(s.E1 - s.E0));
    }
    return WN_OK;
}
// the counters after a planned push, and n_out
static inline void rs_commit_push(RsRow* rows, const RsStep* steps, const int32_t* restart, int32_t B, int32_t* n_out) {
    for (int b = 0; b < B; ++b) {
        const RsStep& s = steps[b];
        n_out[b] = (int32_t)(s.E1 - s.E0);
        if (restart && restart[b]) { rows[b].S = 0; rows[b].ended = false; }
        if (!s.active) continue;
        rows[b].S = s.S1;
        if (s.final) rows[b].ended = true; else rows[b].par ^= 1;      // (a final push stores no tail)
    }
}

// ---- host: one planned row of one push on host arrays.  tail: the inputs [lo(E0), S0); in: the row's n new samples; out receives E1 - E0 samples
static inline void rs_host_push_row(const RsPlan& p, const float* C, const RsStep& s, std::vector<float>* tail, const float* in, float* out) {
    if (s.S0 == 0) tail->clear();      // restarted (or never started): nothing carried
    if (!s.active) return;
    const int64_t lo0 = rs_tail_lo(s.E0, p.L, p.M, p.W);
    std::vector<float> span(*tail);      // the inputs [lo0, S1)
    for (int32_t i = 0; i < s.n; ++i) span.push_back(in[i]);
    for (int64_t m = s.E0; m < s.E1; ++m) out[m - s.E0] = rs_host_output(p, C, span.data(), lo0, s.S1, m);
    if (s.final) { tail->clear(); return; }
    const int64_t lo1 = rs_tail_lo(s.E1, p.L, p.M, p.W);
    tail->assign(span.begin() + (lo1 - lo0), span.end());
}
