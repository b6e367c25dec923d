// Streaming mel analysis: what the device code of wn_mel_stream.hip, the host hook wn_test_mel_stream_plan and the stand-alone host program
// tests/host/mel_stream_main.cpp share -- the geometry, the rule of readiness, and the validation and planning of a push.  Host counters only: nothing here
// touches a device, and the plan runs before any device call.
//
// Notation of wn_mel.hip: off = (n_fft - win_size) / 2, Hl = n_fft / 2 - off, Hr = win_size - Hl.  Frame f reads y[f hop - Hl ... f hop + Hr), y = 0 outside the row.
// A row since its restart: S samples given, F frames analysed.  Not final: the frames f with f hop + Hr <= S are analysed, (S - Hr) / hop + 1 of them (0 for
// S < Hr).  Final: all 1 + S / hop frames, zeros beyond S, as wn_mel_run pads.  What a row carries between pushes:
//   tail    the analysed-domain samples y[T, S), T = max(0, F hop - Hl): exactly those the next frame F reaches back to; fewer than win_size of them
//           (F is not ready: F hop + Hr > S, so S - (F hop - Hl) < Hr + Hl = win_size)
//   carry   the raw sample x[S - 1] for the pre-emphasis of x[S]
//   gain    latched at the restart
// A push of n samples: frames [F, F') are analysed from tail ++ gain (x[s] - k x[s - 1]) of the new samples, F' = ready(S + n, final).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/wavenet_mi355.h"

#define MELS_TILE 32       // new frames per workgroup

struct MelsGeom { int32_t hop = 1, win = 1, Hl = 0, Hr = 0; };

static inline MelsGeom mels_geom(int32_t n_fft, int32_t win_size, int32_t hop) {
    MelsGeom g;
    const int32_t off = (n_fft - win_size) / 2;
    g.hop = hop; g.win = win_size; g.Hl = n_fft / 2 - off; g.Hr = win_size - g.Hl;
    return g;
}

// frames analysed of a row that has consumed S samples since its restart
__host__ __device__ __forceinline__ int64_t mels_ready(const MelsGeom& g, int64_t S, int final) {
    if (final) return 1 + S / g.hop;
    return S >= g.Hr ? (S - g.Hr) / g.hop + 1 : 0;
}
// the first sample frame F reads, clamped to the row: the tail of a row at (S, F) is y[min(mels_tail_lo(F), S), S)
__host__ __device__ __forceinline__ int64_t mels_tail_lo(const MelsGeom& g, int64_t F) {
    const int64_t t = F * g.hop - g.Hl;
    return t > 0 ? t : 0;
}

// (hop > win_size: the next frame may begin beyond the samples given; then nothing is carried)
__host__ __device__ __forceinline__ int64_t mels_tail_at(const MelsGeom& g, int64_t F, int64_t S) {
    const int64_t t = mels_tail_lo(g, F);
    return t < S ? t : S;
}

#define WN_MELS_FAIL(code, ...) do { if (msg && cap > 0) snprintf(msg, (size_t)cap, __VA_ARGS__); return (code); } while (0)

static inline int mels_check_sizes(int32_t max_rows, int32_t max_push, char* msg, int cap) {
    if (max_rows < 0) WN_MELS_FAIL(WN_E_ARG, "max_rows (%d) is negative", max_rows);
    if (max_push < 1) WN_MELS_FAIL(WN_E_ARG, "max_push (%d) must be >= 1", max_push);
    return WN_OK;
}

struct MelsRow { int64_t S = 0, F = 0; float gain = 1.0f; bool ended = false; uint8_t par = 0; };      // par: the tail half the next push reads
// one row of one push, planned from the counters: S0 / F0 after the restart; T0 / T1 the first sample of the tail read / written (tail length S - T)
struct MelsStep { int64_t S0, S1, F0, F1, T0, T1; float gain; int32_t n; uint8_t active, final, par; };

// validates a push and plans every row; changes nothing.  max_rows < 0: no limit on B (the host hook)
static inline int mels_plan_push(const char* who, const MelsGeom& g, int32_t max_rows, int32_t max_push, const MelsRow* rows, const float* in, int64_t in_pitch, const int32_t* n,
                                 const int32_t* restart, const int32_t* final, const float* gain, int32_t B, const float* out, int64_t out_pitch, const int32_t* n_out,
                                 MelsStep* steps, char* msg, int cap) {
    if (!n || !out || !n_out) WN_MELS_FAIL(WN_E_ARG, "%s: null argument", who);
    if (B < 1) WN_MELS_FAIL(WN_E_ARG, "%s: B (%d) must be >= 1", who, B);
    if (max_rows >= 0 && B > max_rows) WN_MELS_FAIL(WN_E_SHAPE, "%s: B (%d) > max_rows = %d", who, B, max_rows);      // (before any of the B entries is read)
    if (in_pitch < 0) WN_MELS_FAIL(WN_E_ARG, "%s: in_pitch (%lld) is negative", who, (long long)in_pitch);
    if (out_pitch < 0) WN_MELS_FAIL(WN_E_ARG, "%s: out_pitch (%lld) is negative", who, (long long)out_pitch);
    bool any = false;
    for (int b = 0; b < B; ++b) {
        if (n[b] < 0) WN_MELS_FAIL(WN_E_ARG, "%s: n[%d] = %d is negative", who, b, n[b]);
        any = any || n[b] > 0;
    }
    if (any && !in) WN_MELS_FAIL(WN_E_ARG, "%s: null argument (in)", who);
    for (int b = 0; b < B; ++b) {
        if (n[b] > max_push) WN_MELS_FAIL(WN_E_SHAPE, "%s: n[%d] = %d > max_push = %d", who, b, n[b], max_push);
        if (n[b] > in_pitch) WN_MELS_FAIL(WN_E_SHAPE, "%s: n[%d] = %d > in_pitch = %lld", who, b, n[b], (long long)in_pitch);
    }
    for (int b = 0; b < B; ++b) {
        MelsStep& s = steps[b];
        const bool rs = restart && restart[b], fin = final && final[b];
        s.n = n[b]; s.final = fin; s.active = n[b] > 0 || fin; s.par = rows[b].par;
        if (s.active && rows[b].ended && !rs) WN_MELS_FAIL(WN_E_STATE, "%s: row %d has ended (final): restart[%d] must be set on its next push", who, b, b);
        s.gain = rs ? (gain ? gain[b] : 1.0f) : rows[b].gain;
        if (rs && !(s.gain == s.gain && s.gain - s.gain == 0.0f)) WN_MELS_FAIL(WN_E_ARG, "%s: gain[%d] = %g is not finite", who, b, (double)s.gain);
        s.S0 = rs ? 0 : rows[b].S; s.F0 = rs ? 0 : rows[b].F;
        s.S1 = s.S0 + n[b];
        if (s.S1 > 0x7fffffffLL) WN_MELS_FAIL(WN_E_SHAPE, "%s: row %d would hold %lld samples since its restart, above 2^31 - 1", who, b, (long long)s.S1);
        s.F1 = s.active ? mels_ready(g, s.S1, fin) : s.F0;
        s.T0 = mels_tail_at(g, s.F0, s.S0); s.T1 = mels_tail_at(g, s.F1, s.S1);
        if (s.F1 - s.F0 > out_pitch) WN_MELS_FAIL(WN_E_SHAPE, "%s: out_pitch (%lld) < n_out[%d] = %lld", who, (long long)out_pitch, b, (long long)(s.F1 - s.F0));
    }
    return WN_OK;
}
// the counters after a planned push, and n_out
static inline void mels_commit_push(MelsRow* rows, const MelsStep* steps, const int32_t* restart, int32_t B, int32_t* n_out) {
    for (int b = 0; b < B; ++b) {
        const MelsStep& s = steps[b];
        n_out[b] = (int32_t)(s.F1 - s.F0);
        if (restart && restart[b]) { rows[b].S = 0; rows[b].F = 0; rows[b].ended = false; rows[b].gain = s.gain; }
        if (!s.active) continue;
        rows[b].S = s.S1; rows[b].F = s.F1;
        if (s.final) rows[b].ended = true; else rows[b].par ^= 1;      // (a final push stores no tail)
    }
}
